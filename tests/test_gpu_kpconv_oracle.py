"""The four KPConv entries ON THE DEVICE against the float64 oracle of tests/kpconv_oracle.py — the mathematics, not another kernel: cbl_kpconv_forward and
cbl_kpconv_forward_ordered (bit-equal), the scatter backward cbl_kpconv_backward (float atomics) and the gather backward cbl_kpconv_backward_csr over three forms
of the transposed table (numpy-built in index order, numpy-built with an order_dst, built by pointops.neighbor_transpose) and the three gradient selections.
Every scene is flip-free with one exact tie placed on purpose, translated far from the origin, has shadow padding, an all-shadow row, a repeated row, a hub of
131 pairs, unlisted targets and an inf in feature row 0 (O.geometry asserts all of it); every entry of every output is compared under the 1e-4 contract
(O.close, which prints the worst ratio); outputs are written over NaN (zeros where the scatter entry accumulates); the gather's workspace has exactly
cbl_kpconv_backward_csr_workspace_bytes bytes.  tests/test_kpconv_oracle_host.py runs the same driver and oracle on the host-emulated kernels.

Which kernel instance a scene takes, and why, is listed at O.EDGE / O.UNALIGNED / O.CAPS.  In short: C % 4 == 0, C <= 64, aligned rows -> kpconv_fwd_c64_kernel
<CLOSEST, LINEAR, ONE = K <= 16>: all eight instances run at the EDGE scenes with C <= 64 (each in the four (influence, mode) combinations, K on both sides of
16) and four of them past the grid cap; C > 64 -> kpconv_fwd_kernel<true> (EDGE C = 68 / 72 / 144, CAPS C = 72); C % 4 != 0 or rows shifted by one float ->
kpconv_fwd_kernel<false>.  kpconv_bwd_kernel (scatter): every scene with K <= 64, BAD_ARG asserted at K = 65 / 130.  kpconv_bwd_csr_kernel<GF, GKW, CLOSEST>:
all six instances at every scene with C % 4 == 0 (UNSUPPORTED asserted otherwise), K = 65 and 130 included.
CAPS: the forward grid is at most 2048 workgroups x 4 points and the gather's at most KB_MAX_GRID = 2048 workgroups x 4 targets per trip, less where fewer
are resident; n = 24611 (> 3 x 8192, no multiple of 32) gives the c64 kernel's three-deep rotation (p0..p3, id0..id2, g0/g1, r0/r1) four trips and more,
n0 = 16501 (> 2 x 8192) gives the gather's two-ahead prefetch three and more — with the `v >= vend` clamps and the holes of the XCD dealing behind them."""
import functools

import numpy as np
import pytest
import torch

from tests import kpconv_oracle as O
from tests.test_gpu_attention import DeviceBackend

pytestmark = pytest.mark.gpu

COMBOS = [(influence, mode) for influence in O.INFLUENCES for mode in O.MODES]
EDGE_RUNS = [shape + combo + (True,) for shape in O.EDGE for combo in COMBOS] + [O.AT_THE_ORIGIN + combo + (False,) for combo in COMBOS]
CAPS_RUNS = [c + (True,) for c in O.CAPS]
RUNS = EDGE_RUNS + CAPS_RUNS
FORMS = ["index order", "ordered", "neighbor_transpose"]
ARGS = "n,n0,K,C,KP,influence,mode,translated"


@pytest.fixture(scope="module")
def entries():
    from contrastboundary_amd import _lib, neighbor_state
    yield O.Entries(_lib.lib(), DeviceBackend())
    neighbor_state.release_unowned_transposes()


class Held:
    """a shape's scene, its float64 results per (influence, mode) and its tables, each computed once per module and left unchanged"""

    def __init__(self, *shape, translated=True):
        self.sc = O.case(*shape, translated=translated)[0]
        self._ref = {}

    def ref(self, influence, mode):
        if (influence, mode) not in self._ref:
            self._ref[influence, mode] = O.reference(self.sc, influence, mode)
        return self._ref[influence, mode]

    @functools.cached_property
    def tables(self):
        """the two numpy tables, and the one cbl_neighbor_transpose builds on the device (no order: the query set is not the support set)"""
        from contrastboundary_amd import pointops
        sc = self.sc
        t = O.tables(sc.idx, sc.n0, sc.seed)
        self.idx_d = torch.from_numpy(sc.idx).cuda()
        t["neighbor_transpose"] = pointops.neighbor_transpose(self.idx_d, sc.n0)
        assert t["neighbor_transpose"] is not None
        return t


@functools.lru_cache(maxsize=None)
def held(n, n0, K, C, KP, translated=True):
    return Held(n, n0, K, C, KP, translated=translated)


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize(ARGS, RUNS)
def test_forward(entries, n, n0, K, C, KP, influence, mode, translated):
    """both entries against the oracle; the ordered entry (a random permutation as `order`) gives the unordered entry's bits"""
    h = held(n, n0, K, C, KP, translated)
    O.check_forward(entries, h.sc, influence, mode, h.ref(influence, mode))


@pytest.mark.parametrize("influence,mode", COMBOS)
def test_forward_with_unaligned_rows(entries, influence, mode):
    """features / out one float past a 16-byte boundary: cbl_kpconv_forward leaves the c64 kernel for kpconv_fwd_kernel<false> (scalar loads) at a shape the c64
    kernel would take; the gather entry refuses such features"""
    h = held(*O.UNALIGNED, True)
    O.check_forward(entries, h.sc, influence, mode, h.ref(influence, mode), shift=1)
    rc, _, _ = entries.gather(h.sc, influence, mode, h.tables["index order"], shift=1)
    assert rc == O.ERR_UNSUPPORTED, rc


# ---------------------------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize(ARGS, RUNS)
def test_scatter_backward(entries, n, n0, K, C, KP, influence, mode, translated):
    """both gradients where K <= 64; CBL_ERR_BAD_ARG at K = 65 and K = 130 (asserted by O.check_scatter)"""
    h = held(n, n0, K, C, KP, translated)
    O.check_scatter(entries, h.sc, influence, mode, h.ref(influence, mode))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize(ARGS, RUNS)
def test_gather_backward(entries, n, n0, K, C, KP, influence, mode, translated, form):
    """both gradients, the features' alone, the kernel weights' alone and both again: values against the oracle, exact zeros for the targets nobody lists
    (one of them holds inf as its feature row), the same bits in every run; CBL_ERR_UNSUPPORTED where C % 4 != 0 (asserted by O.check_gather)"""
    h = held(n, n0, K, C, KP, translated)
    O.check_gather(entries, h.sc, influence, mode, h.ref(influence, mode), h.tables[form], form)


# ---------------------------------------------------------------------------------------------------------------- 3. the autograd wrapper
@pytest.fixture
def counted(monkeypatch):
    from contrastboundary_amd import _lib
    from tests.test_gpu_deterministic import CountingLib
    proxy = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return proxy.calls


@pytest.mark.parametrize("n,n0,K,C,KP,influence,mode", [(50, 80, 17, 64, 15, "linear", "sum"), O.CAPS[3]])
def test_autograd_wrapper(counted, n, n0, K, C, KP, influence, mode):
    """local_aggregation.kpconv(...).backward(...) against the same oracle, and which backward entry it took: the scatter entry below
    pointops.TRANSPOSE_MIN_PAIRS pairs, the gather entry (over the table it builds) from there on"""
    from contrastboundary_amd import local_aggregation, neighbor_state, pointops
    h = held(n, n0, K, C, KP, True)
    sc, (out_ref, gf_ref, gkw_ref) = h.sc, h.ref(influence, mode)
    gathered = n * K >= pointops.TRANSPOSE_MIN_PAIRS
    assert gathered == (n > 1000) and not neighbor_state.is_deterministic()
    d = lambda a: torch.from_numpy(a).cuda()
    f, kw = d(sc.f).requires_grad_(True), d(sc.kw).requires_grad_(True)
    counted.clear()
    out = local_aggregation.kpconv(d(sc.q), d(sc.s), d(sc.idx), f, d(sc.kpts), kw, sc.extent, influence, mode)
    out.backward(d(sc.go))
    torch.cuda.synchronize()
    neighbor_state.release_unowned_transposes()
    tag = "%s %s %s wrapper" % (sc.tag, influence, mode)
    O.close(out.detach().cpu().numpy(), out_ref, tag + " forward")
    O.close(f.grad.cpu().numpy(), gf_ref, tag + " grad features")
    O.close(kw.grad.cpu().numpy(), gkw_ref, tag + " grad kernel_weights")
    taken = {k: v for k, v in counted.items() if k in ("cbl_kpconv_forward", "cbl_kpconv_forward_ordered", "cbl_kpconv_backward", "cbl_kpconv_backward_csr")}
    assert taken == {"cbl_kpconv_forward_ordered": 1, "cbl_kpconv_backward_csr" if gathered else "cbl_kpconv_backward": 1}, counted
