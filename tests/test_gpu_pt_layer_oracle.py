"""The six entries of contrastboundary_amd/csrc/pt_layer.hip ON THE DEVICE against the float64 oracle of tests/pt_layer_oracle.py — the mathematics, not another
kernel of the package: cbl_pt_layer_forward / _forward_eval / _backward (C = 32 | 64, K = 8 | 16) and cbl_pt_layer_wide_forward / _wide_backward /
_wide_backward_csr (C = 128 | 256 | 512).  Every scene is flip-free (O.make_flip_free), every entry of every output is compared under the 1e-4 contract (O.close,
which prints the worst ratio): out, the saved tensors p_r / p0 / p1 / w2 / a, the three BatchNorms' running statistics (three different eps and momenta, buffers
that start from random values and a count of 3), the wide entry's bnc_stats, and all 17 gradients.  Called through ctypes (O.LayerEntries): outputs pre-filled
with NaN, a workspace of exactly the bytes the library asks for, with `order` = NULL and a random permutation.  tests/test_pt_layer_oracle_host.py runs the same
driver and oracle on the host-emulated kernels.

The narrow scenes, (n, K, C).  EDGE: the tile edges of the four (C, K) template instances — (16, 16, 64): the smallest n pt_layer.supported admits, 2 trips on
the 8-workgroup minimum grid, so six workgroups own no tile yet run the in-consumer finalize; (17, 8, 64): 136 pairs, one full trip and half a tile; (41, 8, 32):
n K no multiple of 16; (67, 16, 32): 9 trips, cbl_xcd_per rounds up and virtual slots lie past the end.  CAPS: a workgroup takes 128 pairs per trip, and each n
passes a grid cap of pt_tile_grid / pt_pair_grid / the target pass by a count that is no multiple of a trip — over 256 x 128 pairs (reduce, apply, aggregation
backward, w2 at C = 64: (2100, 16, 64), (4200, 8, 32)), over 512 x 128 (statistics, aggregation forward: (4200, 16, 64), (8300, 8, 64)), over 512 x 256 (the p
chain, its backward, the narrow passes: (8300, 16, 32), (16500, 8, 32)), over 2048 x 16 targets in pt_target_kernel<64, ., 2> ((33000, 8, 64)) and over
2048 x 32 targets in pt_target_kernel<32, ., 3> ((66000, 8, 32)).
The wide scenes: those of tests/test_gpu_attention.py with C >= 128, (520, 16, 512) for pw_logits<64> past 2048 x 256 elements and, forward only and not
flip-free, (5500, 16, 128) for pw_p1 past 1024 x 256 elements.
Measured on an MI355X, the worst error over its bound per entry family: narrow forward 0.0034, evaluation 0.0077, backward 0.0080, PTAttention 0.0072; wide forward
0.0146, backward 0.0172, PTAttentionWide 0.0066 — the kernels' rounding lies two orders of magnitude under the contract, so a subtle defect has room to show."""
import functools

import pytest
import torch

from tests import pt_layer_oracle as O
from tests.test_gpu_attention import DeviceBackend

pytestmark = pytest.mark.gpu

NARROW = O.NARROW_EDGE + O.NARROW_CAPS
WIDE = O.wide_scenes()
ORDERS = ["index order", "ordered"]


@pytest.fixture(scope="module")
def entries():
    from contrastboundary_amd import _lib
    return O.LayerEntries(_lib.lib(), DeviceBackend())


class Scene:
    """a shape's inputs and its float64 results, each computed once per module and left unchanged"""

    def __init__(self, n, K, C):
        self.tag = "(%d, %d, %d)" % (n, K, C)
        self.idx, self.t, self.touched, self.rounds = O.case(n, K, C, flip_free=(n, K, C) != O.WIDE_FORWARD_ONLY)
        self.tables = O.tables(self.idx, self.idx.size)

    @functools.cached_property
    def ref(self):
        return O.reference_layer(self.idx, self.t)

    @functools.cached_property
    def ref_eval(self):
        return O.reference_layer(self.idx, self.t, training=False)


@functools.lru_cache(maxsize=None)
def scene_of(n, K, C):
    return Scene(n, K, C)


# ---------------------------------------------------------------------------------------------------------------- 1. the narrow entries
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,K,C", NARROW)
def test_narrow_forward(entries, n, K, C, order):
    s = scene_of(n, K, C)
    got, _ = entries.forward(s.idx, s.t, s.tables[order][0])
    O.check_forward(got, s.ref, "narrow forward %s %s:" % (s.tag, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,K,C", NARROW)
def test_narrow_backward(entries, n, K, C, order):
    """the 17 gradients from what the device's own forward call saved (its constants block has no other source); d x_k / d x_v are gathers written over a NaN
    fill, exact zeros for the target nobody lists"""
    s = scene_of(n, K, C)
    _, kept = entries.forward(s.idx, s.t, s.tables[order][0])
    O.check_backward(entries.backward(s.idx, s.t, kept, s.tables[order]), s.ref, "narrow backward %s %s:" % (s.tag, order), True)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,K,C", O.NARROW_EVAL)
def test_narrow_forward_evaluation(entries, n, K, C, order):
    """cbl_pt_layer_forward_eval against the evaluation formula with the same (random) running statistics, which stay bit-unchanged"""
    s = scene_of(n, K, C)
    got, _ = entries.forward(s.idx, s.t, s.tables[order][0], "eval")
    O.check_eval(got, s.ref_eval, s.t, "narrow eval %s %s:" % (s.tag, order))


# ---------------------------------------------------------------------------------------------------------------- 2. the wide entries
@pytest.mark.parametrize("n,K,C", WIDE)
def test_wide_forward(entries, n, K, C):
    s = scene_of(n, K, C)
    got, _ = entries.forward(s.idx, s.t, mode="wide")
    O.check_forward(got, s.ref, "wide forward %s:" % s.tag)


def test_wide_forward_past_the_p1_grid(entries):
    """(5500, 16, 128): 264000 elements of p1, pw_p1_kernel's 1024 workgroups of 256 take a second trip.  Forward only, so the scene is not made flip-free (a
    ReLU is continuous: a pre-activation near zero moves no output by more than its own rounding)"""
    s = scene_of(*O.WIDE_FORWARD_ONLY)
    got, _ = entries.forward(s.idx, s.t, mode="wide")
    O.check_forward(got, s.ref, "wide forward %s:" % s.tag)


@pytest.mark.parametrize("form", ["scatter", "csr, index order", "csr, ordered"])
@pytest.mark.parametrize("n,K,C", WIDE)
def test_wide_backward(entries, n, K, C, form):
    """cbl_pt_layer_wide_backward (float atomics into d x_k / d x_v, which the call zeroes itself: they are NaN before it) and cbl_pt_layer_wide_backward_csr
    (gathers over the transposed table, without and with an order)"""
    s = scene_of(n, K, C)
    _, kept = entries.forward(s.idx, s.t, mode="wide")
    table = None if form == "scatter" else s.tables[form[5:]]
    got = entries.backward(s.idx, s.t, kept, table, "wide scatter" if table is None else "wide csr")
    O.check_backward(got, s.ref, "wide backward %s %s:" % (s.tag, form), table is not None)


# ---------------------------------------------------------------------------------------------------------------- 3. refused calls
def test_refused_calls(entries):
    """a misaligned x_q / w2 / idx, a workspace one byte short, a K or C outside the entry's set, the gather backward without its tables: the entry's error code,
    and every NaN-filled output and every BatchNorm buffer as it was"""
    O.check_arguments(entries, wide=False)
    O.check_arguments(entries, wide=True)


# ---------------------------------------------------------------------------------------------------------------- 4. the autograd wrappers
BACKWARD_ENTRIES = {"cbl_pt_layer_backward", "cbl_pt_layer_wide_backward", "cbl_pt_layer_wide_backward_csr"}


@pytest.fixture
def counted(monkeypatch):
    from contrastboundary_amd import _lib
    from tests.test_gpu_deterministic import CountingLib
    proxy = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return proxy.calls


def _through_the_wrapper(function, s, tag, gathered):
    d = {k: torch.from_numpy(s.t[k]).cuda().requires_grad_(k in O.FEATURES + O.PARAMS) for k in ["xyz", "g_out"] + O.FEATURES + O.PARAMS}
    idx = torch.from_numpy(s.idx).cuda()
    bns = []
    for q, width in enumerate((3, s.t["gamma_c"].size, s.t["gamma_g"].size)):
        bn = torch.nn.BatchNorm1d(width, eps=O.EPS3[q], momentum=O.MOMENTUM3[q]).cuda().train()
        with torch.no_grad():
            bn.running_mean.copy_(torch.from_numpy(s.t["run_mean%d" % q])); bn.running_var.copy_(torch.from_numpy(s.t["run_var%d" % q]))
            bn.num_batches_tracked.fill_(O.COUNT0)
        bns.append(bn)
    out = function.apply(d["xyz"], d["x_q"], d["x_k"], d["x_v"], idx, tuple(bns), *[d[k] for k in O.PARAMS])
    (out * d["g_out"]).sum().backward()
    torch.cuda.synchronize()
    O.close(out.detach().cpu().numpy(), s.ref["out"], tag + " out")
    for q, bn in enumerate(bns):
        O.close(bn.running_mean.cpu().numpy(), s.ref["run_mean"][q], "%s running mean of %s" % (tag, O.BN_NAMES[q]))
        O.close(bn.running_var.cpu().numpy(), s.ref["run_var"][q], "%s running variance of %s" % (tag, O.BN_NAMES[q]))
        assert int(bn.num_batches_tracked) == O.COUNT0 + 1
    O.check_backward({k: d[k].grad.cpu().numpy() for k in O.FEATURES + O.PARAMS}, s.ref, tag, gathered)


def test_narrow_autograd_wrapper(counted):
    """pt_layer.PTAttention (its own spatial order, its own transposed table) against the same oracle, and the backward entry it took"""
    from contrastboundary_amd import neighbor_state, pt_layer
    s = scene_of(4200, 16, 64)
    counted.clear()
    _through_the_wrapper(pt_layer.PTAttention, s, "narrow wrapper %s:" % s.tag, True)
    neighbor_state.release_unowned_transposes()
    assert {k: v for k, v in counted.items() if k in BACKWARD_ENTRIES} == {"cbl_pt_layer_backward": 1}, counted


@pytest.mark.parametrize("switch", [False, True])
def test_wide_autograd_wrapper(counted, switch):
    """pt_layer.PTAttentionWide with the deterministic switch off (the scatter entry) and on (the gather entry)"""
    from contrastboundary_amd import neighbor_state, pt_layer
    s = scene_of(800, 16, 256)
    assert not neighbor_state.is_deterministic()
    counted.clear()
    with neighbor_state.deterministic(switch):
        _through_the_wrapper(pt_layer.PTAttentionWide, s, "wide wrapper %s, switch %s:" % (s.tag, "on" if switch else "off"), switch)
    assert not neighbor_state.is_deterministic()
    neighbor_state.release_unowned_transposes()
    want = "cbl_pt_layer_wide_backward_csr" if switch else "cbl_pt_layer_wide_backward"
    assert {k: v for k, v in counted.items() if k in BACKWARD_ENTRIES} == {want: 1}, counted
