"""CPU: the pool_bn kernels (contrastboundary_amd/csrc/pool_bn.hip: TF batch norm + activation over (rows, C) rows, the step behind every local aggregation of
the ConvNet) compiled for the HOST and run with wave semantics (tests/host_emul/wave), through their C entry points, against the float64 restatement in the
direct form (tests/pool_bn_oracle.py): every entry within 1e-4 of its column's scale.  The workspace is poisoned with 0xff and every output with NaN before
each call.  Gradient cases with relu or leaky_relu assert, from the oracle, that no pre-activation can flip between fp32 and float64.
A stand-alone AddressSanitizer program (tests/host_emul/pool_bn_asan_main.cpp) runs the same translation unit over the shape edges with heap buffers of
exactly their documented size: an indexing error of a kernel surfaces there, on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pool_bn_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, run_sanitizer_program, sanitizer_program

cf = ctypes.c_float
ll = ctypes.c_longlong
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def host():
    return load("pool_bn", ["pool_bn"])


def odd_slice(a):
    """a copy of `a` (rows, C) that is rows 1.. of a 16-byte aligned (rows + 1, C) array: with C odd its base is not 16-byte aligned"""
    big = aligned(np.zeros((a.shape[0] + 1, a.shape[1]), np.float32))
    view = big[1:]
    view[...] = a
    assert view.flags["C_CONTIGUOUS"]
    return view


def run(L, case, bn="batch", activation="relu", backward=True, momentum=0.98, eps=1e-3, place=aligned):
    """forward (+ backward) through the C entry points -> dict(out, the gradients, moving_mean, moving_var, save_mean, save_invstd, raw = every array a
    call wrote).  place: where the (rows, C) arrays live (aligned, or odd_slice)"""
    x, go = place(case["x"]), place(case["go"])
    rows, C = x.shape
    bn_mode = {"batch": 1, "moving": 2, None: 0}[bn]
    v = lambda key: aligned(case[key]) if bn_mode else None
    gamma, beta, mm, mv = v("gamma"), v("beta"), v("moving_mean"), v("moving_var")
    save_mean, save_invstd = (nans(C), nans(C)) if bn_mode else (None, None)
    act = O.ACTIVATIONS[activation]
    nbytes = L.cbl_pool_bn_workspace_bytes(ll(rows), C)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    nan_rows = lambda: place(np.full((rows, C), np.nan, np.float32))
    out = nan_rows()
    rc = L.cbl_pool_bn_forward(ll(rows), C, P(x), bn_mode, P(gamma), P(beta), cf(eps), cf(momentum), P(mm), P(mv), act, P(save_mean), P(save_invstd), P(out),
                               P(ws), ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res = dict(out=out, raw=[out] + ([save_mean, save_invstd, mm, mv] if bn_mode else []))
    if bn_mode:
        res.update(moving_mean=mm, moving_var=mv, save_mean=save_mean, save_invstd=save_invstd)
    if not backward:
        return res
    g_x = nan_rows()
    g_gamma, g_beta = (nans(C), nans(C)) if bn_mode else (None, None)
    ws[...] = 0xff                                                   # (nothing of the forward's workspace is needed)
    rc = L.cbl_pool_bn_backward(ll(rows), C, P(x), bn_mode, P(gamma), P(save_mean), P(save_invstd), act, P(out), P(go), P(g_x), P(g_gamma), P(g_beta), P(ws),
                                ctypes.c_size_t(nbytes), None)
    assert rc == 0
    res["grad_x"] = g_x
    res["raw"].append(g_x)
    if bn_mode:
        res.update(grad_gamma=g_gamma, grad_beta=g_beta)
        res["raw"] += [g_gamma, g_beta]
    return res


def written(res):
    assert all(np.isfinite(a).all() for a in res["raw"])             # written, not accumulated: nothing of the NaN fill is left


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("activation", sorted(O.ACTIVATIONS))
def test_every_bn_mode_and_activation(host, bn, activation):
    """the base shape: out, the three gradients and the moving statistics; evaluation leaves the moving statistics alone"""
    case = O.make_case(*O.BASE, O.SEED)
    ref = O.reference(case, bn, activation)
    O.assert_flip_free(ref, activation)
    res = run(host, case, bn, activation)
    O.check(res, ref, bn, "%s %s" % (bn, activation))
    written(res)
    if bn == "moving":
        np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
        np.testing.assert_array_equal(res["moving_var"], case["moving_var"])
        np.testing.assert_array_equal(res["save_mean"], case["moving_mean"])


@pytest.mark.parametrize("rows,C", O.SHAPES)
def test_shapes(host, rows, C):
    """O.SHAPES: rows 1, 2, 63, 64, 65, both sides of the single-launch rule, every width class — gradients with the identity (no flip possible) under
    batch statistics, forward with relu, and the moving statistics with leaky_relu forward"""
    case = O.make_case(rows, C, 3)
    res = run(host, case, "batch", "none")
    O.check(res, O.reference(case, "batch", "none"), "batch", "batch")
    written(res)
    O.check(run(host, case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")
    O.check(run(host, case, "moving", "leaky_relu", backward=False), O.reference(case, "moving", "leaky_relu", backward=False), "moving", "moving")


@pytest.mark.parametrize("rows,C", O.CAP_SHAPES)
def test_more_rows_than_the_grid_cap(host, rows, C):
    """O.CAP_SHAPES: the chunked kernels (pb_stats_kernel, pb_normalize_kernel, pb_sums_kernel, pb_dx_kernel) share one grid (chunks, slabs) whose cap is
    PB_MAX_CHUNKS = 512 chunks: past it a chunk holds more than one fetch per row lane.  (The finalize kernels' grids are ceil(C / 32) and ceil(C / 256):
    at most 128 workgroups at the widest C, no cap.)"""
    assert rows > O.PB_MAX_CHUNKS * O.row_lanes(C, False) * O.PB_BATCH
    case = O.make_case(rows, C, 6)
    res = run(host, case, "batch", "none")
    O.check(res, O.reference(case, "batch", "none"), "batch", "cap")
    written(res)


def test_an_unaligned_base(host):
    """documented: no alignment beyond a float's is required.  A row slice of an odd-width tensor (C = 3, C = 7): the base is 12 / 28 bytes past a 16-byte
    boundary; and C = 72 four bytes past one (a width that could be vectorised, a base that cannot)"""
    for rows, C, place in ((150, 3, odd_slice), (1100, 7, odd_slice), (150, 72, lambda a: aligned(a, 4))):
        case = O.make_case(rows, C, 4)
        assert place(case["x"]).ctypes.data % 16 != 0
        for bn in O.BNS:
            res = run(host, case, bn, "none", place=place)
            O.check(res, O.reference(case, bn, "none"), bn, "unaligned %s" % bn)
            written(res)


@pytest.mark.parametrize("rows", [300, 3000])                        # the single launch, the chunked launches
def test_ill_conditioned_columns(host, rows):
    """|mean| / std up to 1e4 and an exactly constant column: centred statistics keep every digit the float32 mean leaves; the bound is derived in
    tests/pool_bn_oracle.reference (`floors`).  The uncentred formula E[x^2] - E[x]^2, substituted in the oracle in float32, FAILS the same check (asserted once, here, on the CPU)."""
    C = 24
    case = O.ill_case(rows, C, 11)
    ref = O.reference(case, "batch", "none")
    floors = ref["floors"]
    res = run(host, case, "batch", "none")
    O.check(res, ref, "batch", "ill-conditioned %d" % rows)
    written(res)
    # the share of the error that the mean's rounding explains: |out - ref| over the floor, on the columns of ratio 1e4 (the figure of the profile)
    hard = [c for c in range(C) if c % 4 == 3]
    err = np.abs(res["out"].astype(np.float64) - ref["out"])[:, hard].max(0)
    print("ill-conditioned, rows %d: worst |out - ref| / (eps32 |mean| invstd |gamma|) on the 1e4 columns: %.3f" % (rows, float((err / floors["out"][hard]).max())))
    assert (err <= floors["out"][hard]).all()                        # ... and there the floor ALONE holds
    # forward with relu (the error is continuous through the activation)
    fwd = O.reference(case, "batch", "relu", backward=False)
    O.check(run(host, case, "batch", "relu", backward=False), fwd, "batch", "ill-conditioned relu")
    # the constant column: variance exactly 0, out exactly beta, invstd exactly eps^-1/2
    np.testing.assert_array_equal(res["out"][:, 5], np.full(rows, case["beta"][5], np.float32))
    assert res["save_invstd"][5] == np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-3)))) and res["save_mean"][5] == np.float32(12345.678)
    # the uncentred formula in float32 does not pass
    bad = O.reference(case, "batch", "none", uncentred=True, dtype=torch.float32)
    with pytest.raises(AssertionError):
        O.check(bad, ref, "batch", "uncentred")


def test_moving_statistics_and_one_row(host):
    """TF's update with another momentum; rows == 1: variance 0, invstd = eps^-1/2, out = beta; rows == 0 and bn_mode 2 write no buffer"""
    case = O.make_case(200, 12, 1)
    ref = O.reference(case, "batch", "none", momentum=0.9, eps=1e-5)
    res = run(host, case, "batch", "none", momentum=0.9, eps=1e-5)
    O.check(res, ref, "batch", "momentum 0.9")
    np.testing.assert_allclose(res["save_invstd"], ref["save_invstd"], rtol=1e-5)
    one = O.make_case(1, 12, 2)
    res = run(host, one, "batch", "none", eps=1e-3)
    assert (res["save_invstd"] == np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-3))))).all()
    np.testing.assert_array_equal(res["save_mean"], one["x"][0])
    np.testing.assert_array_equal(res["out"][0], one["beta"])
    np.testing.assert_allclose(res["moving_var"], one["moving_var"] * np.float32(0.98), rtol=1e-6)   # the batch variance is 0
    # without moving statistics (both NULL) under bn_mode 1
    x, gamma, beta = aligned(case["x"]), aligned(case["gamma"]), aligned(case["beta"])
    rows, C = x.shape
    nbytes = host.cbl_pool_bn_workspace_bytes(ll(rows), C)
    ws, sm, si, out = aligned(np.zeros(nbytes, np.uint8)), nans(C), nans(C), nans(rows, C)
    assert host.cbl_pool_bn_forward(ll(rows), C, P(x), 1, P(gamma), P(beta), cf(1e-5), cf(0.9), None, None, 0, P(sm), P(si), P(out), P(ws),
                                    ctypes.c_size_t(nbytes), None) == 0
    np.testing.assert_array_equal(out, run(host, case, "batch", "none", momentum=0.9, eps=1e-5, backward=False)["out"])
    # rows == 0: nothing is written
    mm, mv = aligned(case["moving_mean"]), aligned(case["moving_var"])
    sm[...] = np.nan
    assert host.cbl_pool_bn_forward(ll(0), C, None, 1, P(gamma), P(beta), cf(1e-3), cf(0.98), P(mm), P(mv), 1, P(sm), P(si), None, None, 0, None) == 0
    np.testing.assert_array_equal(mm, case["moving_mean"]); np.testing.assert_array_equal(mv, case["moving_var"])
    assert not np.isfinite(sm).any()


def test_two_calls_give_identical_bits(host):
    for rows in (300, 1100):
        case = O.make_case(rows, 72, 0)
        for bn, activation in (("batch", "relu"), ("moving", "leaky_relu"), (None, "none")):
            a = run(host, case, bn, activation)["raw"]
            b = run(host, case, bn, activation)["raw"]
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_single_gradients_have_the_bits_of_the_full_call(host):
    """any gradient may be NULL: each alone gives the bits it has beside the others"""
    for rows in (300, 1100):
        case = O.make_case(rows, 20, 2)
        full = run(host, case, "batch", "leaky_relu")
        x, go, gamma = aligned(case["x"]), aligned(case["go"]), aligned(case["gamma"])
        C = x.shape[1]
        nbytes = host.cbl_pool_bn_workspace_bytes(ll(rows), C)
        ws = aligned(np.full(nbytes, 0xff, np.uint8))
        for key in ("grad_x", "grad_gamma", "grad_beta"):
            g = nans(rows, C) if key == "grad_x" else nans(C)
            args = [P(g) if k == key else None for k in ("grad_x", "grad_gamma", "grad_beta")]
            ws[...] = 0xff
            assert host.cbl_pool_bn_backward(ll(rows), C, P(x), 1, P(gamma), P(full["save_mean"]), P(full["save_invstd"]), 2, P(full["out"]), P(go), *args, P(ws),
                                             ctypes.c_size_t(nbytes), None) == 0
            np.testing.assert_array_equal(g.view(np.uint32), full[key].view(np.uint32))


def test_unsupported_and_bad_arguments(host):
    """C = 4097: CBL_ERR_UNSUPPORTED (-3) and a workspace size of 0; a NULL input, a mode out of range, gamma missing under bn_mode 1: CBL_ERR_BAD_ARG
    (-1); a workspace one byte short: CBL_ERR_WORKSPACE (-2) — all before any launch; rows == 0: a no-op"""
    rows, C = 40, 12
    case = O.make_case(rows, C, 0)
    x, go, gamma, beta = aligned(case["x"]), aligned(case["go"]), aligned(case["gamma"]), aligned(case["beta"])
    size = host.cbl_pool_bn_workspace_bytes
    nbytes = size(ll(rows), C)
    ws = aligned(np.zeros(nbytes, np.uint8))
    out, sm, si = nans(rows, C), nans(C), nans(C)
    mm, mv = aligned(case["moving_mean"]), aligned(case["moving_var"])

    def fwd(rows=rows, C=C, x=x, bn_mode=1, gamma=gamma, act=1, out=out, nbytes=nbytes, mm=None, mv=None, eps=1e-3):
        return host.cbl_pool_bn_forward(ll(rows), C, P(x), bn_mode, P(gamma), P(beta), cf(eps), cf(0.98), P(mm), P(mv), act, P(sm), P(si), P(out), P(ws),
                                        ctypes.c_size_t(nbytes), None)
    assert fwd(C=4097) == -3
    assert size(ll(rows), 4097) == 0 and size(ll(rows), 4096) > 0 and size(ll(-1), C) == 0 and size(ll(rows), 0) == 0
    assert fwd(x=None) == -1 and fwd(out=None) == -1 and fwd(gamma=None) == -1 and fwd(bn_mode=3) == -1 and fwd(bn_mode=-1) == -1 and fwd(act=3) == -1
    assert fwd(C=0) == -1 and fwd(rows=-1) == -1 and fwd(eps=0.0) == -1
    assert fwd(mm=mm) == -1                                          # a moving mean without a moving variance
    assert fwd(bn_mode=2) == -1                                      # evaluation without moving statistics
    assert fwd(nbytes=nbytes - 1) == -2
    assert fwd(rows=0) == 0
    assert not np.isfinite(out).any() and not np.isfinite(sm).any()  # nothing was launched
    assert fwd(bn_mode=0, gamma=None, nbytes=0) == 0 and np.isfinite(out).all()      # bn=False needs neither variables nor a workspace
    assert fwd(mm=mm, mv=mv) == 0
    g_x, g_g = nans(rows, C), nans(C)

    def bwd(C=C, x=x, go=go, bn_mode=1, act=1, out=out, nbytes=nbytes, g_g=None, rows=rows, gamma=gamma):
        return host.cbl_pool_bn_backward(ll(rows), C, P(x), bn_mode, P(gamma), P(sm), P(si), act, P(out), P(go), P(g_x), P(g_g), None, P(ws),
                                         ctypes.c_size_t(nbytes), None)
    assert bwd(C=4097) == -3
    assert bwd(x=None) == -1 and bwd(go=None) == -1 and bwd(out=None) == -1 and bwd(gamma=None) == -1 and bwd(bn_mode=3) == -1 and bwd(act=-1) == -1
    assert bwd(bn_mode=0, g_g=g_g) == -1                             # grad_gamma without a batch norm
    assert bwd(nbytes=nbytes - 1) == -2
    assert bwd(rows=0) == 0
    assert not np.isfinite(g_x).any() and not np.isfinite(g_g).any()
    assert bwd(g_g=g_g) == 0 and np.isfinite(g_x).all() and np.isfinite(g_g).all()
    assert bwd(bn_mode=0, out=None, act=0, x=None, gamma=None, nbytes=0) == 0        # the identity: grad_x = grad_out
    np.testing.assert_array_equal(g_x, go)


def test_the_kernels_under_address_sanitizer():
    """the stand-alone program: the same translation unit with -fsanitize=address,undefined, forward + backward over the shape edges, heap buffers of exactly
    their documented size"""
    r = run_sanitizer_program(sanitizer_program("pool_bn", ["pool_bn"]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
