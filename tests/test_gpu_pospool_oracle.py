"""The three PosPool entries ON THE DEVICE against the float64 oracle of tests/pospool_oracle.py — the mathematics, not another kernel and not the fp32
restatement, whose sine argument carries the kernels' own rounding: cbl_pospool_forward, the scatter backward cbl_pospool_backward (float atomics) and the gather
backward cbl_pospool_backward_csr over three forms of the transposed table (numpy-built in index order, numpy-built with an order_dst, built by
pointops.neighbor_transpose), and the autograd wrapper with the entry it chooses.  Every scene is translated far from the origin, has shadow padding, an
all-shadow row, a repeated row, a hub of 131 pairs, unlisted targets with inf in their feature rows, is flip-free for 'max' with one exact tie between two
different neighbours and one all-negative channel beside shadow entries, and keeps the rounding of the inputs under 2e-5 (O.geometry asserts all of it); every
entry of every output is compared under the 1e-4 contract taken per row (O.close, which prints the worst ratio); outputs are written over NaN (zeros where the
scatter entry accumulates); the gather's workspace has exactly cbl_pospool_backward_csr_workspace_bytes(n) bytes.  This is also the only place where v_sin_f32 on
up to 16 turns meets the mathematical sine: the host emulation and the fp32 restatement both use the library's.  tests/test_pospool_oracle_host.py runs the same
driver and oracle on the host-emulated kernels.

Which kernel instance a scene takes, and why, is listed at O.EDGE / O.UNALIGNED / O.CAPS.  CAPS: pospool_fwd_v4 is capped at 8192 workgroups (8209 and 8204
trips), pospool_bwd_csr_kernel at 2048 (4133 trips: three passes, also through an order_dst), pospool_kernel at 4096 workgroups x 4 waves (16421 points: a
wave's LDS rows are reused behind the closing wave_barrier), pospool_inv_count_kernel at 4096 x 256 points (1048583) — with the `v < vend` loops and the holes of
the XCD dealing (`p >= n`, `tr >= n0`) behind them."""
import functools

import numpy as np
import pytest
import torch

from tests import pospool_oracle as O
from tests.test_gpu_attention import DeviceBackend

pytestmark = pytest.mark.gpu

EDGE_RUNS = [shape + (r, True) for shape in O.EDGE for r in O.REDUCTIONS] + [O.AT_THE_ORIGIN + (r, False) for r in O.REDUCTIONS]
CAPS_RUNS = [c + (True,) for c in O.CAPS]
RUNS = EDGE_RUNS + CAPS_RUNS
FORMS = ["index order", "ordered", "neighbor_transpose"]
ARGS = "n,n0,K,C,pe,reduction,translated"
CAPS_REDUCTIONS = {c[:5]: (c[5],) for c in O.CAPS}


@pytest.fixture(scope="module")
def entries():
    from contrastboundary_amd import _lib, neighbor_state
    yield O.Entries(_lib.lib(), DeviceBackend())
    neighbor_state.release_unowned_transposes()


class Held:
    """a shape's scene (which holds its float64 results per reduction), its tables and its gather results over the table in index order, each computed once per
    module and left unchanged"""

    def __init__(self, *shape, translated=True, padded=True, reductions=O.REDUCTIONS):
        self.sc = O.case(*shape, translated=translated, padded=padded, reductions=reductions)
        self._gathered = {}

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

    def in_index_order(self, E, reduction):
        if reduction not in self._gathered:
            rc, gf = E.gather(self.sc, self.sc.pe, reduction, self.tables["index order"])
            assert rc == O.OK, rc
            self._gathered[reduction] = gf
        return self._gathered[reduction]


@functools.lru_cache(maxsize=None)
def held(n, n0, K, C, pe, translated=True, padded=True):
    return Held(n, n0, K, C, pe, translated=translated, padded=padded, reductions=CAPS_REDUCTIONS.get((n, n0, K, C, pe), O.REDUCTIONS if padded else ("mean",)))


# ---------------------------------------------------------------------------------------------------------------- 1. the entries
@pytest.mark.parametrize(ARGS, RUNS)
def test_forward(entries, n, n0, K, C, pe, reduction, translated):
    """values; for 'max' also -65535 in the all-shadow row and a real, negative maximum in the all-negative channel of a padded row"""
    O.check_forward(entries, held(n, n0, K, C, pe, translated).sc, reduction)


@pytest.mark.parametrize(ARGS, RUNS)
def test_scatter_backward(entries, n, n0, K, C, pe, reduction, translated):
    """all three reductions, K up to 128; exact zeros for the targets nobody lists"""
    O.check_scatter(entries, held(n, n0, K, C, pe, translated).sc, reduction)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize(ARGS, RUNS)
def test_gather_backward(entries, n, n0, K, C, pe, reduction, translated, form):
    """values against the oracle, exact zeros written over NaN for the targets nobody lists (two of them hold inf as their feature rows), the same bits in a
    second run and as over the table in index order; CBL_ERR_UNSUPPORTED for 'max' and C % 4 != 0, CBL_ERR_BAD_ARG for a workspace one byte short and for
    gradients one float past a 16-byte boundary (all asserted by O.check_gather)"""
    h = held(n, n0, K, C, pe, translated)
    same = h.in_index_order(entries, reduction) if form != "index order" and reduction != "max" and C % 4 == 0 else None
    O.check_gather(entries, h.sc, reduction, h.tables[form], form, same_bits=same)


@pytest.mark.parametrize("reduction", O.REDUCTIONS)
def test_unaligned(entries, reduction):
    """features / out one float past a 16-byte boundary: cbl_pospool_forward leaves pospool_fwd_v4 for pospool_kernel<false> (scalar loads) at a shape the vector
    kernel would take, and stays within the contract; the gather entry refuses such gradients"""
    h = held(*O.UNALIGNED)
    O.check_forward(entries, h.sc, reduction, shift=1)
    rc, _ = entries.gather(h.sc, h.sc.pe, reduction, h.tables["index order"], shift=1)
    assert rc == (O.ERR_UNSUPPORTED if reduction == "max" else O.ERR_BAD_ARG), rc


@pytest.mark.parametrize("n,n0,K,C,pe", O.NO_PADDING)
def test_mean_quirk_without_padding(entries, n, n0, K, C, pe):
    """no entry equals n0: padding_num is the largest REAL index listed; its entries contribute but are not counted, and the row made of it alone is divided by
    1e-5 — forward, scatter and gather"""
    h = held(n, n0, K, C, pe, True, False)
    sc = h.sc
    assert not sc.padded and sc.padding_num < n0 and (sc.idx == sc.padding_num).any()
    O.check_forward(entries, sc, "mean")
    O.check_scatter(entries, sc, "mean")
    O.check_gather(entries, sc, "mean", h.tables["index order"], "index order")
    big = np.abs(sc.ref["mean"][0]).max(1)
    assert big[sc.shadow_row] > 1e4 * np.median(big)


@pytest.mark.parametrize("n,n0,K,C,pe", [(40, 60, 17, 72, "sin_cos"), (39, 58, 20, 64, "exp_-d"), (120, 48, 3, 12, "xyz"), (29, 90, 128, 36, "sin_cos")])
def test_max_ties(entries, n, n0, K, C, pe):
    """the gradient shared by tied maxima: the K entries of the repeated row, and two DIFFERENT neighbours whose products are both exactly 0 while every
    other product of that (p, c) is negative"""
    O.check_max_ties(entries, held(n, n0, K, C, pe).sc)


def test_refusals(entries):
    """CBL_ERR_BAD_ARG at K = 129 = PP_KMAX + 1, CBL_ERR_UNSUPPORTED at 'sin_cos' with C = 10, from all three entries"""
    O.check_refusals(entries)


def test_empty_support(entries):
    """n0 = 0, n = 37: zeros for 'sum' / 'mean', -65535 for 'max', status 0.  cbl_pospool_forward takes its vector kernel only where n0 > 0: that kernel loads
    row 0 of features / support_points for a shadow entry before it skips it, which an empty buffer does not have"""
    O.check_empty_support(entries)
    # through the wrapper, where the empty features / support_points tensors have no address at all (torch: data_ptr() == 0)
    from contrastboundary_amd import local_aggregation
    sc = O.empty_support(37, 3, 12, "sin_cos")
    d = lambda a: torch.from_numpy(a).cuda()
    for reduction, value in (("sum", 0.0), ("mean", 0.0), ("max", O.SHADOW_MAX)):
        f = d(sc.f).requires_grad_(True)
        out = local_aggregation.pospool(d(sc.q), d(sc.s), d(sc.idx), f, float(sc.radius), sc.pe, reduction)
        out.backward(d(sc.go))
        assert (out.detach().cpu().numpy() == np.float32(value)).all() and f.grad.shape == (0, 12), reduction


# ---------------------------------------------------------------------------------------------------------------- 2. the autograd wrapper
@pytest.fixture
def counted(monkeypatch):
    from contrastboundary_amd import _lib
    from tests.test_gpu_deterministic import CountingLib
    proxy = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return proxy.calls


@pytest.mark.parametrize("n,n0,K,C,pe,reduction,entry", [(40, 60, 17, 72, "sin_cos", "mean", "cbl_pospool_backward"),        # under TRANSPOSE_MIN_PAIRS
                                                         (16421, 6007, 9, 36, "sin_cos", "max", "cbl_pospool_backward"),      # 'max', 147789 pairs
                                                         (16421, 6007, 9, 9, "sin_cos", "mean", "cbl_pospool_backward"),      # C % 4 != 0, 147789 pairs
                                                         (24611, 300, 4, 264, "xyz", "mean", "cbl_pospool_backward_csr")])    # 98444 pairs
def test_autograd_wrapper(counted, n, n0, K, C, pe, reduction, entry):
    """local_aggregation.pospool(...).backward(...) against the same oracle, and which backward entry it took: the scatter entry below
    pointops.TRANSPOSE_MIN_PAIRS pairs, for 'max' and for C % 4 != 0, the gather entry (over the table it builds) otherwise; reduction 'avg' gives the bits
    of 'mean' (the forward's always, the gradient's where the gather entry wrote it: the scatter entry's float atomics have no fixed order)"""
    from contrastboundary_amd import local_aggregation, neighbor_state, pointops
    sc = held(n, n0, K, C, pe).sc
    out_ref, gf_ref = sc.ref[reduction]
    many = n * K >= pointops.TRANSPOSE_MIN_PAIRS
    assert many == (n > 1000) and not neighbor_state.is_deterministic()
    assert entry == ("cbl_pospool_backward_csr" if many and reduction != "max" and C % 4 == 0 else "cbl_pospool_backward")
    d = lambda a: torch.from_numpy(a).cuda()
    results = {}
    for name in (reduction, "avg") if reduction == "mean" else (reduction,):
        f = d(sc.f).requires_grad_(True)
        counted.clear()
        out = local_aggregation.pospool(d(sc.q), d(sc.s), d(sc.idx), f, float(sc.radius), pe, name)
        out.backward(d(sc.go))
        torch.cuda.synchronize()
        neighbor_state.release_unowned_transposes()
        taken = {k: v for k, v in counted.items() if k in ("cbl_pospool_forward", "cbl_pospool_backward", "cbl_pospool_backward_csr")}
        assert taken == {"cbl_pospool_forward": 1, entry: 1}, counted
        results[name] = out.detach().cpu().numpy(), f.grad.cpu().numpy()
    tag = "%s %s wrapper" % (sc.tag, reduction)
    O.close(results[reduction][0], out_ref, tag + " forward")
    O.close(results[reduction][1], gf_ref, tag + " grad features")
    if "avg" in results:
        assert np.array_equal(O.bits(results["avg"][0]), O.bits(results["mean"][0])), tag + ": 'avg' forward"
        O.close(results["avg"][1], gf_ref, tag + " 'avg' grad features")
        if entry == "cbl_pospool_backward_csr":
            assert np.array_equal(O.bits(results["avg"][1]), O.bits(results["mean"][1])), tag + ": 'avg' grad features"
