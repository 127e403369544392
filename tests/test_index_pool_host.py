"""CPU: the gradient kernels of ind_max_pool (contrastboundary_amd/csrc/index_pool.hip; tensorflow/models/basic_operators.py:155-172) compiled for the HOST and
run with wave semantics (tests/host_emul/wave), through their C entry point, behind the product's own forward (cbl_ind_max_pool, whose column-minimum keys the
backward reads) and the product's own table (cbl_neighbor_transpose); ind_closest_pool's gradient (models/heads/seg_head.py:13-28) as the mirror computes it,
cbl_grouping_backward_csr_rows over the table of the first column.  Against the float64 torch composition of tests/index_pool_oracle.py (a restatement:
TensorFlow is absent) within the 1e-4 contract; grad_x is pre-filled with NaN (every row must be written)."""
import ctypes

import numpy as np
import pytest

from tests import index_pool_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans


@pytest.fixture(scope="module")
def host():
    return load("index_pool", ["local_aggregation", "index_pool", "neighbor_transpose"])


def table(L, inds, n1):
    """cbl_neighbor_transpose of inds over n1 targets -> inv_start, inv_src"""
    n2, k = inds.shape
    inv_start, inv_src = np.full(n1 + 1, -1, np.int32), np.full(max(n2 * k, 1), -1, np.int32)
    nbytes = L.cbl_neighbor_transpose_workspace_bytes(n2, n1, k)
    ws = aligned(np.zeros(max(nbytes, 16), np.uint8))
    assert L.cbl_neighbor_transpose(n2, n1, k, P(inds), None, None, P(inv_start), P(inv_src), P(ws), ctypes.c_size_t(nbytes), None) == 0
    return inv_start, inv_src


def forward_max(L, x, inds):
    n1, d = x.shape
    n2, k = inds.shape
    keymin, out = np.zeros(d, np.uint32), nans(n2, d)
    assert L.cbl_ind_max_pool(n1, n2, k, d, P(x), P(inds), P(keymin), P(out), None) == 0
    return keymin, out


def backward_max(L, case, off=0):
    """-> out, grad_x through the C entries; off = 4: rows that are not 16-byte aligned (the one-channel kernels whatever d is)"""
    x, inds, g = aligned(case["x"], off), np.ascontiguousarray(case["inds"]), aligned(case["g"], off)
    n1, d = x.shape
    n2, k = inds.shape
    keymin, out = forward_max(L, x, inds)
    inv_start, inv_src = table(L, inds, n1)
    nbytes = L.cbl_ind_max_pool_backward_workspace_bytes(n1, n2, k, d)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    grad = nans(n1, d)
    rc = L.cbl_ind_max_pool_backward_csr(n1, n2, k, d, P(x), P(inds), P(keymin), P(out), P(g), None, P(inv_start), P(inv_src), P(grad), P(ws),
                                         ctypes.c_size_t(nbytes), None)
    assert rc == 0
    return out, grad


def backward_closest(L, case):
    inds, g = case["inds"], aligned(case["g"])
    n1, d = case["x"].shape
    inds0 = np.ascontiguousarray(inds[:, :1])
    inv_start, inv_src = table(L, inds0, n1)
    grad = nans(n1, d)
    assert L.cbl_grouping_backward_csr_rows(n1, d, d, 0, P(g), None, P(inv_start), P(inv_src), P(grad), None) == 0
    return grad


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F"])
def test_the_restated_gradient_is_the_autograd_of_the_composition(name):
    """the oracle checked against the explicit formulas of cbl_amd.h (both float64; they differ by the order of their sums only)"""
    case = O.make_case(name)
    out, grad = O.reference_max(name)
    r_out, r_grad = O.restated_max(case)
    np.testing.assert_array_equal(out, r_out)
    np.testing.assert_allclose(grad, r_grad, rtol=0, atol=1e-12 * np.abs(grad).max())


@pytest.mark.parametrize("name", O.QUANTISED + ("C",))
def test_the_tie_cases_have_ties(name):
    O.assert_tied(O.make_case(name))


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F"])
def test_ind_max_pool_gradient(host, name):
    case = O.make_case(name)
    if name in O.QUANTISED:
        O.assert_tied(case)
    ref_out, ref_grad = O.reference_max(name)
    out, grad = backward_max(host, case)
    np.testing.assert_array_equal(out, ref_out.astype(np.float32))       # elements of x: exact
    assert np.isfinite(grad).all()
    O.close(grad, ref_grad, name)


@pytest.mark.parametrize("name", ["B", "C"])
def test_unaligned_rows_take_the_one_channel_kernels(host, name):
    case = O.make_case(name)
    out, grad = backward_max(host, case, off=4)
    np.testing.assert_array_equal(out, O.reference_max(name)[0].astype(np.float32))
    O.close(grad, O.reference_max(name)[1], name)


def test_unreferenced_source_rows_get_exact_zeros(host):
    case = O.make_case("E")
    assert not np.isin(np.arange(30, 50), case["inds"]).any() and (case["inds"] == 50).any()
    _, grad = backward_max(host, case)
    assert (grad[30:] == 0).all() and np.abs(grad[:30]).max() > 0
    gc = backward_closest(host, case)
    assert (gc[30:] == 0).all()
    O.close(gc, O.reference_closest("E")[1])                            # up to 20 references per source row


def test_closest_pool_gradient_with_single_references_is_exact(host):
    case = O.make_case("E1")
    first = case["inds"][:, 0]
    real = first[first < 500]
    assert len(np.unique(real)) == len(real) and len(real) < len(first)
    gc = backward_closest(host, case)
    np.testing.assert_array_equal(gc, O.reference_closest("E1")[1].astype(np.float32))


def test_two_calls_give_identical_bits(host):
    for name in ("B", "D"):
        a, b = backward_max(host, O.make_case(name))[1], backward_max(host, O.make_case(name))[1]
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_return_codes(host):
    """-1 bad argument, -2 short workspace, -3 unsupported, before any launch; n2 == 0 writes zeros"""
    case = O.make_case("C")
    x, inds, g = aligned(case["x"]), np.ascontiguousarray(case["inds"]), aligned(case["g"])
    n1, d = x.shape
    n2, k = inds.shape
    keymin, out = forward_max(host, x, inds)
    inv_start, inv_src = table(host, inds, n1)
    nbytes = host.cbl_ind_max_pool_backward_workspace_bytes(n1, n2, k, d)
    ws = aligned(np.zeros(nbytes, np.uint8))
    grad = nans(n1, d)

    def bwd(n1=n1, n2=n2, k=k, d=d, x=x, inds=inds, keymin=keymin, out=out, g=g, inv_start=inv_start, inv_src=inv_src, grad=grad, ws=ws, nbytes=nbytes):
        return host.cbl_ind_max_pool_backward_csr(n1, n2, k, d, P(x), P(inds), P(keymin), P(out), P(g), None, P(inv_start), P(inv_src), P(grad), P(ws),
                                                  ctypes.c_size_t(nbytes), None)
    assert bwd(n1=0) == -1 and bwd(n2=-1) == -1 and bwd(k=0) == -1 and bwd(d=0) == -1
    for missing in ("x", "inds", "keymin", "out", "g", "inv_start", "inv_src", "grad", "ws"):
        assert bwd(**{missing: None}) == -1, missing
    assert bwd(nbytes=nbytes - 1) == -2 and bwd(nbytes=0) == -2
    assert bwd(n2=1 << 30, k=4) == -3
    assert host.cbl_ind_max_pool_backward_workspace_bytes(n1, 1 << 30, 4, d) == 0 and host.cbl_ind_max_pool_backward_workspace_bytes(0, n2, k, d) == 0
    assert np.isnan(grad).all()                                          # nothing ran
    assert bwd(n2=0, x=None, inds=None, g=None, out=None, ws=None, nbytes=0) == 0
    assert (grad == 0).all()
    assert bwd() == 0
    O.close(grad, O.reference_max("C")[1])
