"""GPU: ind_max_pool / ind_closest_pool / nearest_upsample with gradients (contrastboundary_amd/local_aggregation over csrc/index_pool.hip and the transposed
table; tensorflow/models/basic_operators.py:155-192, models/heads/seg_head.py:13-28) through the Python mirror with `out.backward(g)`, against the float64 torch
composition of tests/index_pool_oracle.py (a restatement: TensorFlow is absent) within the 1e-4 contract.  The cases of tests/test_index_pool_host.py on the device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import index_pool_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def run(op, case):
    """-> out, grad_x (torch, on the device) of op(x, inds) under out.backward(g)"""
    x = dev(case["x"]).requires_grad_(True)
    out = op(x, dev(case["inds"]))
    out.backward(dev(case["g"]))
    return out.detach(), x.grad


def forward_entry(case):
    """the existing forward entry, called directly"""
    from contrastboundary_amd import _lib
    x, inds = dev(case["x"]), dev(case["inds"])
    (n1, d), (n2, k) = x.shape, inds.shape
    scratch = torch.empty(d, dtype=torch.int32, device="cuda")
    out = torch.empty((n2, d), dtype=torch.float32, device="cuda")
    i = ctypes.c_int
    _lib.check(_lib.lib().cbl_ind_max_pool(i(n1), i(n2), i(k), i(d), _lib.ptr(x), _lib.ptr(inds), _lib.ptr(scratch), _lib.ptr(out), _lib.stream_of(x)), "cbl_ind_max_pool")
    return out


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F"])
def test_ind_max_pool_gradient(name):
    from contrastboundary_amd import local_aggregation as LA
    case = O.make_case(name)
    if name in O.QUANTISED:
        O.assert_tied(case)
    ref_out, ref_grad = O.reference_max(name)
    out, grad = run(LA.ind_max_pool, case)
    assert torch.equal(out, forward_entry(case))                         # the differentiable path leaves the forward's bits alone
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out.astype(np.float32))
    g = grad.cpu().numpy()
    print(name, "max |grad - ref| / max |ref| = %.3e" % (np.abs(g - ref_grad).max() / np.abs(ref_grad).max()))
    assert np.isfinite(g).all()
    O.close(g, ref_grad, name)
    assert torch.equal(run(LA.ind_max_pool, case)[1], grad)              # two calls: the same bits


def test_no_gradient_was_there_before():
    """what fails on the forward-only operators: autograd through ind_max_pool, and the C entries of its gradient"""
    from contrastboundary_amd import _lib, local_aggregation as LA
    case = O.make_case("C")
    x = dev(case["x"]).requires_grad_(True)
    gx, = torch.autograd.grad(LA.ind_max_pool(x, dev(case["inds"])).sum(), x)
    assert gx.shape == x.shape
    assert hasattr(_lib.lib(), "cbl_ind_max_pool_backward_csr") and hasattr(_lib.lib(), "cbl_ind_max_pool_backward_workspace_bytes")


def test_a_column_slice_of_wider_rows_takes_the_one_channel_kernels():
    """rows that are not 16-byte aligned (a tensor starting one float into its storage) behind the same function"""
    from contrastboundary_amd import local_aggregation as LA
    case = O.make_case("B")
    n1, d = case["x"].shape
    flat = torch.zeros(n1 * d + 1, device="cuda")
    x = flat[1:].view(n1, d)
    x.copy_(dev(case["x"]))
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    x.requires_grad_(True)
    out = LA.ind_max_pool(x, dev(case["inds"]))
    gx, = torch.autograd.grad(out, x, dev(case["g"]))
    O.close(gx.cpu().numpy(), O.reference_max("B")[1])


@pytest.mark.parametrize("name", ["E", "E1", "B"])
def test_closest_pool_and_nearest_upsample_gradient(name):
    from contrastboundary_amd import local_aggregation as LA
    case = O.make_case(name)
    n1 = case["x"].shape[0]
    ref_out, ref_grad = O.reference_closest(name)
    for op in (LA.ind_closest_pool, LA.nearest_upsample):
        out, grad = run(op, case)
        np.testing.assert_array_equal(out.cpu().numpy(), ref_out.astype(np.float32))
        first = torch.from_numpy(np.array(case["inds"][:, 0])).long()
        real = (first >= 0) & (first < n1)
        cpu = torch.zeros(case["x"].shape).index_add_(0, first[real], torch.from_numpy(np.array(case["g"]))[real])      # float32, in row order
        if name == "E1":                                                 # at most one reference per source row: nothing is summed
            assert torch.equal(grad.cpu(), cpu)
        else:
            O.close(grad.cpu().numpy(), ref_grad, name)
            torch.testing.assert_close(grad.cpu(), cpu, rtol=1e-4, atol=1e-4 * float(cpu.abs().max()))
        assert torch.equal(run(op, case)[1], grad)


def test_unreferenced_source_rows_get_exact_zeros():
    from contrastboundary_amd import local_aggregation as LA
    case = O.make_case("E")
    assert not np.isin(np.arange(30, 50), case["inds"]).any() and (case["inds"] == 50).any()
    for op in (LA.ind_max_pool, LA.ind_closest_pool):
        grad = run(op, case)[1]
        assert bool((grad[30:] == 0).all()) and float(grad[:30].abs().max()) > 0


def test_forward_and_backward_in_a_replayed_graph():
    """case B captured once after a warm-up call that builds and registers the transposed table (no allocation or synchronisation inside the entries),
    replayed twice: equal to the eager call bit for bit"""
    from contrastboundary_amd import local_aggregation as LA
    case = O.make_case("B")
    x, inds, g = dev(case["x"]).requires_grad_(True), dev(case["inds"]), dev(case["g"])

    def step():
        out = LA.ind_max_pool(x, inds)
        gx, = torch.autograd.grad(out, x, g)
        return out, gx
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                           # the warm-up's stream: the registered table needs no cross-stream wait
        out = step()
    for t in out:
        t.detach().zero_()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    O.close(out[1].cpu().numpy(), O.reference_max("B")[1])
