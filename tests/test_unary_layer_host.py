"""CPU: the unary layer's kernels (contrastboundary_amd/csrc/unary_layer.hip; tensorflow/models/basic_operators.py:195-241) compiled for the HOST and run with
wave semantics (tests/host_emul/wave: the MFMA chain is emulated in its own lane layout), through their C entry points, against the float64 restatement of
the graph code (tests/unary_layer_oracle.py) within the 1e-4 contract.  The workspace is poisoned with 0xff and every output with NaN before each call.
Gradient cases with relu or leaky_relu assert, from the oracle, that no pre-activation can flip between fp32 and float64 (seeds chosen so).
A stand-alone AddressSanitizer program (tests/host_emul/unary_layer_asan_main.cpp) runs the same translation unit over the shape edges with heap buffers of
exactly their documented size: an indexing error of a kernel surfaces there, on the CPU."""
import ctypes

import numpy as np
import pytest

from tests import unary_layer_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, run_sanitizer_program, sanitizer_program

cf = ctypes.c_float
ll = ctypes.c_longlong


@pytest.fixture(scope="module")
def host():
    return load("unary_layer", ["unary_layer"])


def run(L, case, bn="batch", activation="relu", shortcut=True, bias=True, backward=True, momentum=0.98, eps=1e-3, off=0):
    """forward (+ backward) through the C entry points -> dict(out, y, the gradients, moving_mean, moving_var, raw = every array a call wrote).
    off = 4: every (rows, .) array and the weights start 4 bytes past a 16-byte boundary"""
    x, W, go = aligned(case["x"], off), aligned(case["W"], off), aligned(case["go"], off)
    rows, c_in = x.shape
    c_out = W.shape[1]
    b = aligned(case["biases"]) if bias else None
    sc = aligned(case["shortcut"], off) if shortcut else None
    bn_mode = {"batch": 1, "moving": 2, None: 0}[bn]
    v = lambda key: aligned(case[key]) if bn_mode else None
    gamma, beta, mm, mv = v("gamma"), v("beta"), v("moving_mean"), v("moving_var")
    save_mean, save_invstd = (nans(c_out), nans(c_out)) if bn_mode else (None, None)
    act = O.ACTIVATIONS[activation]
    nbytes = L.cbl_unary_layer_workspace_bytes(ll(rows), c_in, c_out)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    nan_rows = lambda c: aligned(np.full((rows, c), np.nan, np.float32), off)
    y, out = nan_rows(c_out), nan_rows(c_out)
    rc = L.cbl_unary_layer_forward(ll(rows), c_in, c_out, P(x), P(W), P(b), P(sc), bn_mode, P(gamma), P(beta), cf(eps), cf(momentum), P(mm), P(mv), act,
                                   P(save_mean), P(save_invstd), P(y), P(out), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res = dict(out=out, y=y, raw=[out, y] + ([save_mean, save_invstd, mm, mv] if bn_mode else []))
    if bn_mode:
        res.update(moving_mean=mm, moving_var=mv)
    if not backward:
        return res
    g_x, g_W = nan_rows(c_in), aligned(np.full((c_in, c_out), np.nan, np.float32), off)
    g_b = nans(c_out) if bias else None
    g_gamma, g_beta = (nans(c_out), nans(c_out)) if bn_mode else (None, None)
    g_sc = nan_rows(c_out) if shortcut else None
    ws[...] = 0xff                                                   # (nothing of the forward's workspace is needed)
    rc = L.cbl_unary_layer_backward(ll(rows), c_in, c_out, P(x), P(W), bn_mode, P(gamma), P(save_mean), P(save_invstd), act, P(y), P(out), P(go), P(g_x), P(g_W),
                                    P(g_b), P(g_gamma), P(g_beta), P(g_sc), P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res.update(grad_x=g_x, grad_W=g_W)
    for key, g in (("grad_biases", g_b), ("grad_gamma", g_gamma), ("grad_beta", g_beta), ("grad_shortcut", g_sc)):
        if g is not None:
            res[key] = g
            res["raw"].append(g)
    res["raw"] += [g_x, g_W]
    return res


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("activation", sorted(O.ACTIVATIONS))
def test_every_bn_mode_activation_shortcut_and_bias(host, bn, activation):
    """the base shape: out, y, all six gradients and the moving statistics; evaluation leaves the moving statistics alone"""
    case = O.base_case()
    for sc in (True, False):
        for bias in (True, False):
            ref = O.reference(case, bn, activation, sc, bias)
            O.assert_flip_free(ref, activation)
            res = run(host, case, bn, activation, sc, bias)
            O.check(res, ref, bn, "%s %s shortcut %s bias %s" % (bn, activation, sc, bias))
            assert all(np.isfinite(a).all() for a in res["raw"])     # written, not accumulated: nothing of the NaN fill is left
            if bn == "moving":
                np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
                np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


@pytest.mark.parametrize("rows,c_in,c_out", O.EDGES)
def test_tile_edges(host, rows, c_in, c_out):
    """one below, at and one above the 64-wide tile in each of the three dimensions, one row, c_in = 5, c_out = 13: gradients with the identity (no flip
    possible), forward with relu; batch statistics with shortcut and bias, and the bare product with a bias (segmentation_pred)"""
    case = O.make_case(rows, c_in, c_out, 3)
    O.check(run(host, case, "batch", "none"), O.reference(case, "batch", "none"), "batch", "batch")
    O.check(run(host, case, None, "none", shortcut=False), O.reference(case, None, "none", shortcut=False), None, "bare")
    O.check(run(host, case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


def test_a_base_pointer_offset_by_4_bytes_works(host):
    """documented: no alignment beyond a float's is required (the scalar-load path)"""
    case = O.base_case()
    for bn in O.BNS:
        ref = O.reference(case, bn, "leaky_relu")
        O.assert_flip_free(ref, "leaky_relu")
        O.check(run(host, case, bn, "leaky_relu", off=4), ref, bn, "offset %s" % bn)


@pytest.mark.parametrize("rows,c_in,c_out", O.CHUNKS)
def test_weight_gradient_chunks(host, rows, c_in, c_out):
    case = O.make_case(rows, c_in, c_out, 5)
    for bn in ("batch", None):
        O.check(run(host, case, bn, "none"), O.reference(case, bn, "none"), bn, str(bn))


@pytest.mark.parametrize("rows,c_in,c_out", O.CAPS)
def test_more_tiles_and_trips_than_every_grid_cap(host, rows, c_in, c_out):
    """O.CAPS: the first shape walks past the cap of the row-tile kernels and of the column sums, the second past the cap of the elementwise passes"""
    case = O.make_case(rows, c_in, c_out, 6)
    O.check(run(host, case, "batch", "none"), O.reference(case, "batch", "none"), "batch")


@pytest.mark.parametrize("rows,c_in,c_out", O.EXTREMES)
def test_the_networks_extremes(host, rows, c_in, c_out):
    case = O.make_case(rows, c_in, c_out, 7)
    O.check(run(host, case, "batch", "none"), O.reference(case, "batch", "none"), "batch")
    O.check(run(host, case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


def test_column_means_near_8(host):
    """|mean y| is many standard deviations of y: a variance by E[y^2] - E[y]^2 in fp32 would leave no digits (centred tile partials, fp64 combine)"""
    case = O.make_case(*O.BASE, O.SEED_MEAN_8, mean_8=True)
    y = O.reference(case, "batch", "relu", False, False, backward=False)["y"]
    assert 4 < np.abs(y.mean(0)).min() and 0.5 < y.std(0).min() and y.std(0).max() < 2.5
    for sc, bias in ((False, False), (True, True)):
        ref = O.reference(case, "batch", "relu", sc, bias)
        O.assert_flip_free(ref, "relu")
        O.check(run(host, case, "batch", "relu", sc, bias), ref, "batch")


def test_two_calls_give_identical_bits(host):
    case = O.make_case(1100, 36, 72, 0)
    for bn, activation in (("batch", "relu"), ("moving", "leaky_relu"), (None, "none")):
        a = run(host, case, bn, activation)["raw"]
        b = run(host, case, bn, activation)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_grad_biases_alone_and_grad_weights_alone(host):
    """grad_biases without grad_weights launches only the row of tiles that sums dy's columns; each alone gives the bits it has beside the other, with one
    chunk of rows and with several"""
    for rows in (150, 1100):
        case = O.make_case(rows, 70, 72, 2)
        full = run(host, case, "batch", "none")
        x, W, go, gamma = (aligned(case[k]) for k in ("x", "W", "go", "gamma"))
        c_in, c_out = W.shape
        nbytes = host.cbl_unary_layer_workspace_bytes(ll(rows), c_in, c_out)
        ws = aligned(np.full(nbytes, 0xff, np.uint8))
        sm, si = nans(c_out), nans(c_out)
        y, out = nans(rows, c_out), nans(rows, c_out)
        assert host.cbl_unary_layer_forward(ll(rows), c_in, c_out, P(x), P(W), P(aligned(case["biases"])), P(aligned(case["shortcut"])), 1, P(gamma),
                                            P(aligned(case["beta"])), cf(1e-3), cf(0.98), None, None, 0, P(sm), P(si), P(y), P(out), P(ws),
                                            ctypes.c_size_t(nbytes), None) == 0
        for want_w, want_b in ((False, True), (True, False)):
            g_W, g_b = (nans(c_in, c_out) if want_w else None), (nans(c_out) if want_b else None)
            ws[...] = 0xff
            assert host.cbl_unary_layer_backward(ll(rows), c_in, c_out, P(x), P(W), 1, P(gamma), P(sm), P(si), 0, P(y), P(out), P(go), None, P(g_W), P(g_b), None,
                                                 None, None, P(ws), ctypes.c_size_t(nbytes), None) == 0
            if want_w:
                np.testing.assert_array_equal(g_W.view(np.uint32), full["grad_W"].view(np.uint32))
            if want_b:
                np.testing.assert_array_equal(g_b.view(np.uint32), full["grad_biases"].view(np.uint32))


def test_unsupported_and_bad_arguments(host):
    """outside the limits: CBL_ERR_UNSUPPORTED (-3) and a workspace size of 0; a NULL input: CBL_ERR_BAD_ARG (-1); a workspace one byte short:
    CBL_ERR_WORKSPACE (-2) — all before any launch; rows == 0: a no-op"""
    rows, c_in, c_out = 40, 8, 12
    case = O.make_case(rows, c_in, c_out, 0)
    x, W, go, gamma, beta = case["x"], case["W"], case["go"], case["gamma"], case["beta"]
    size = host.cbl_unary_layer_workspace_bytes
    nbytes = size(ll(rows), c_in, c_out)
    ws = aligned(np.zeros(nbytes, np.uint8))
    y, out, sm, si = nans(rows, c_out), nans(rows, c_out), nans(c_out), nans(c_out)

    def fwd(rows=rows, c_in=c_in, c_out=c_out, x=x, bn_mode=1, gamma=gamma, act=1, y=y, nbytes=nbytes, mm=None):
        return host.cbl_unary_layer_forward(ll(rows), c_in, c_out, P(x), P(W), None, None, bn_mode, P(gamma), P(beta), cf(1e-3), cf(0.98), P(mm), None, act, P(sm),
                                            P(si), P(y), P(out), P(ws), ctypes.c_size_t(nbytes), None)
    assert fwd(c_out=4097) == -3 and fwd(c_in=4097) == -3
    assert size(ll(rows), c_in, 4097) == 0 and size(ll(rows), 4097, c_out) == 0 and size(ll(rows), 4096, 4096) > 0
    assert fwd(x=None) == -1 and fwd(gamma=None) == -1 and fwd(y=None) == -1 and fwd(bn_mode=3) == -1 and fwd(act=3) == -1 and fwd(c_in=0) == -1
    assert fwd(mm=case["moving_mean"]) == -1                         # a moving mean without a moving variance
    assert fwd(bn_mode=2) == -1                                      # evaluation without moving statistics
    assert fwd(nbytes=nbytes - 1) == -2
    assert fwd(rows=0) == 0
    assert not np.isfinite(out).any() and not np.isfinite(y).any() and not np.isfinite(sm).any()      # nothing was launched
    assert fwd() == 0
    g_x, g_W, g_g = nans(rows, c_in), nans(c_in, c_out), nans(c_out)

    def bwd(c_out=c_out, x=x, go=go, bn_mode=1, out=out, nbytes=nbytes, g_g=None, rows=rows):
        return host.cbl_unary_layer_backward(ll(rows), c_in, c_out, P(x), P(W), bn_mode, P(gamma), P(sm), P(si), 1, P(y), P(out), P(go), P(g_x), P(g_W), None, P(g_g),
                                             None, None, P(ws), ctypes.c_size_t(nbytes), None)
    assert bwd(c_out=4097) == -3
    assert bwd(x=None) == -1 and bwd(go=None) == -1 and bwd(out=None) == -1
    assert bwd(bn_mode=0, g_g=g_g) == -1                             # grad_gamma without a batch norm
    assert bwd(nbytes=nbytes - 1) == -2
    assert bwd(rows=0) == 0
    assert not np.isfinite(g_x).any() and not np.isfinite(g_W).any() and not np.isfinite(g_g).any()
    assert bwd(g_g=g_g) == 0 and np.isfinite(g_x).all() and np.isfinite(g_W).all() and np.isfinite(g_g).all()


def test_the_kernels_under_address_sanitizer():
    """the stand-alone program: the same translation unit with -fsanitize=address,undefined, forward + backward over the shape edges, heap buffers of exactly
    their documented size"""
    r = run_sanitizer_program(sanitizer_program("unary_layer", ["unary_layer"]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
