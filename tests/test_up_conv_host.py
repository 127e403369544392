"""CPU: the segmentation head's decoder step (cbl_up_conv_*, contrastboundary_amd/csrc/up_conv.hip; tensorflow/models/heads/seg_head.py:63-67) compiled for
the HOST and run with wave semantics (tests/host_emul/wave), through its C entry points, against the float64 restatement of the graph code in its direct form
(tests/up_conv_oracle.py: gather, concat, unary layer) within the 1e-4 contract.  The workspace is poisoned with 0xff and every output with NaN before each
call: an output that was accumulated into, or not written, stays NaN.  Gradient cases with relu or leaky_relu assert, from the oracle, that no
pre-activation can flip between fp32 and float64.  A stand-alone AddressSanitizer program (tests/host_emul/up_conv_asan_main.cpp) runs the same translation
units over the shape edges with heap buffers of exactly their documented size; nothing is loaded into Python under a sanitizer."""
import ctypes

import numpy as np
import pytest

from tests import up_conv_oracle as O
from tests.host_emul.host_build import P, aligned, load, nans, run_sanitizer_program, sanitizer_program

FILES = ["up_conv", "neighbor_transpose"]                           # the entries, and cbl_grouping_backward_csr_rows (the segment sum)
cf = ctypes.c_float
ll = ctypes.c_longlong
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def host():
    return load("up_conv", FILES)


def first_column_table(inds, n1):
    """cbl_neighbor_transpose's output for the table's first column (n2 sources, ONE column) over n1 targets, restated: inv_start (n1 + 1), inv_src = per
    coarse row the ascending list of the fine rows it is the nearest of; shadow ids (outside [0, n1)) are in no list"""
    first = inds[:, 0].astype(np.int64)
    keep = np.nonzero((first >= 0) & (first < n1))[0]
    order = np.argsort(first[keep], kind="stable")
    inv_start = np.zeros(n1 + 1, np.int64)
    np.add.at(inv_start, first[keep] + 1, 1)
    return np.cumsum(inv_start).astype(np.int32), np.ascontiguousarray(keep[order].astype(np.int32))


def run(L, case, bn="batch", activation="relu", bias=True, backward=True, momentum=0.98, eps=1e-3, off=0, want=None):
    """forward (+ backward) through the C entry points -> dict(out, y, the gradients, moving_mean, moving_var, raw = every array a call wrote).
    off = 4: every feature array and the weights start 4 bytes past a 16-byte boundary; want: the gradients asked for (all by default)"""
    coarse, skip, W, go = (aligned(case[key], off) for key in ("coarse", "skip", "W", "go"))
    inds = np.ascontiguousarray(case["inds"])
    (n2, k), (n1, c_up), c_skip, c_out = inds.shape, coarse.shape, skip.shape[1], W.shape[1]
    b = aligned(case["biases"]) if bias else None
    bn_mode = {"batch": 1, "moving": 2, None: 0}[bn]
    v = lambda key: aligned(case[key]) if bn_mode else None
    gamma, beta, mm, mv = v("gamma"), v("beta"), v("moving_mean"), v("moving_var")
    save_mean, save_invstd = (nans(c_out), nans(c_out)) if bn_mode else (None, None)
    act = O.ACTIVATIONS[activation]
    nbytes = L.cbl_up_conv_workspace_bytes(ll(n2), ll(n1), c_up, c_skip, c_out)
    assert nbytes > 0
    ws = aligned(np.full(nbytes, 0xff, np.uint8))
    nan_rows = lambda r, c: aligned(np.full((r, c), np.nan, np.float32), off)
    y, out = nan_rows(n2, c_out), nan_rows(n2, c_out)
    rc = L.cbl_up_conv_forward(ll(n2), ll(n1), c_up, c_skip, c_out, P(coarse), P(inds), k, P(skip), P(W), P(b), bn_mode, P(gamma), P(beta), cf(eps), cf(momentum),
                               P(mm), P(mv), act, P(save_mean), P(save_invstd), P(y), P(out), P(ws), sz(nbytes), None)
    assert rc == 0
    res = dict(out=out, y=y, raw=[out, y] + ([save_mean, save_invstd, mm, mv] if bn_mode else []))
    if bn_mode:
        res.update(moving_mean=mm, moving_var=mv)
    if not backward:
        return res
    inv_start, inv_src = first_column_table(inds, n1)
    asked = lambda key: want is None or key in want
    g = dict(grad_coarse=nan_rows(n1, c_up) if asked("grad_coarse") else None, grad_skip=nan_rows(n2, c_skip) if asked("grad_skip") else None,
             grad_W=aligned(np.full(W.shape, np.nan, np.float32), off) if asked("grad_W") else None,
             grad_biases=nans(c_out) if bias and asked("grad_biases") else None,
             grad_gamma=nans(c_out) if bn_mode and asked("grad_gamma") else None, grad_beta=nans(c_out) if bn_mode and asked("grad_beta") else None)
    ws[...] = 0xff                                                   # (nothing of the forward's workspace is needed)
    rc = L.cbl_up_conv_backward(ll(n2), ll(n1), c_up, c_skip, c_out, P(coarse), P(inds), k, P(skip), P(W), bn_mode, P(gamma), P(save_mean), P(save_invstd), act,
                                P(y), P(out), P(go), None, P(inv_start), P(inv_src), P(g["grad_coarse"]), P(g["grad_skip"]), P(g["grad_W"]), P(g["grad_biases"]),
                                P(g["grad_gamma"]), P(g["grad_beta"]), P(ws), sz(nbytes), None)
    assert rc == 0
    for key, a in g.items():
        if a is not None:
            res[key] = a
            res["raw"].append(a)
    return res


def written(res):
    assert all(np.isfinite(a).all() for a in res["raw"])             # written, not accumulated: nothing of the NaN fill is left


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("activation", sorted(O.ACTIVATIONS))
def test_every_bn_mode_activation_and_bias(host, bn, activation):
    """the base shape and table (shadow ids, a row nobody references, a hub of 131 rows; columns 1 and 2 hold other valid ids): out, y, all gradients and
    the moving statistics; evaluation leaves the moving statistics alone"""
    case = O.base_case()
    for bias in (True, False):
        ref = O.reference(case, bn, activation, bias)
        O.assert_flip_free(ref, activation)
        res = run(host, case, bn, activation, bias)
        O.check(res, ref, bn, "%s %s bias %s" % (bn, activation, bias))
        written(res)
        assert (res["grad_coarse"][O.UNREFERENCED] == 0).all()       # exact zeros for the coarse row nobody references
        if bn == "moving":
            np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
            np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


def edge_case(L, shape, seed=3):
    """gradients with the identity (no flip possible) under batch statistics and as the bare product with a bias, forward with relu"""
    case = O.make_case(*shape, seed)
    for res, ref, bn in ((run(L, case, "batch", "none"), O.reference(case, "batch", "none"), "batch"),
                         (run(L, case, None, "none"), O.reference(case, None, "none"), None),
                         (run(L, case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch")):
        O.check(res, ref, bn, str(bn))
        written(res)


@pytest.mark.parametrize("shape", O.EDGES + O.ODD)
def test_tile_edges_and_odd_widths(host, shape):
    edge_case(host, shape)


def test_a_table_of_shadow_ids_only(host):
    """every fine row reads the zero row: grad_coarse is all zeros, grad_W's upper block too, and coarse @ W_up goes unused"""
    case = O.make_case(*O.BASE, 4, kind="shadow")
    res = run(host, case, "batch", "none")
    O.check(res, O.reference(case, "batch", "none"), "batch")
    written(res)
    assert (res["grad_coarse"] == 0).all() and (res["grad_W"][:O.BASE[2]] == 0).all()


def test_bases_offset_by_4_bytes(host):
    """documented: no alignment beyond a float's is required (the scalar-load path)"""
    case = O.base_case()
    for bn in O.BNS:
        ref = O.reference(case, bn, "leaky_relu")
        O.assert_flip_free(ref, "leaky_relu")
        O.check(run(host, case, bn, "leaky_relu", off=4), ref, bn, "offset %s" % bn)


@pytest.mark.parametrize("shape", O.CHUNKS)
def test_weight_gradient_chunks(host, shape):
    case = O.make_case(*shape, 5)
    for bn in ("batch", None):
        res = run(host, case, bn, "none")
        O.check(res, O.reference(case, bn, "none"), bn, str(bn))
        written(res)


@pytest.mark.parametrize("shape", O.CAPS)
def test_more_tiles_and_trips_than_every_grid_cap(host, shape):
    case = O.make_case(*shape, 6)
    O.check(run(host, case, "batch", "none"), O.reference(case, "batch", "none"), "batch")


@pytest.mark.parametrize("shape", O.SPLITS)
def test_split_contraction_on_both_sides_of_its_rule(host, shape):
    edge_case(host, shape, seed=8)


@pytest.mark.parametrize("shape", O.EXTREMES)
def test_the_heads_extremes(host, shape):
    case = O.make_case(*shape, 7)
    O.check(run(host, case, "batch", "none"), O.reference(case, "batch", "none"), "batch")
    O.check(run(host, case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


def test_two_calls_give_identical_bits(host):
    case = O.multi_case()
    for bn, activation in (("batch", "relu"), ("moving", "leaky_relu"), (None, "none")):
        a = run(host, case, bn, activation)["raw"]
        b = run(host, case, bn, activation)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_each_gradient_alone_has_the_bits_it_has_beside_the_others(host):
    """any gradient may be NULL; one chunk of rows and several"""
    for n2, n1 in ((150, 40), (1100, 600)):
        case = O.make_case(n2, n1, 36, 36, 72, 2, 2)
        full = run(host, case, "batch", "none")
        for key in ("grad_coarse", "grad_skip", "grad_W", "grad_biases", "grad_gamma"):
            alone = run(host, case, "batch", "none", want=(key,))
            assert [k for k in alone if k.startswith("grad_")] == [key]
            np.testing.assert_array_equal(alone[key].view(np.uint32), full[key].view(np.uint32), err_msg=key)


def test_unsupported_and_bad_arguments(host):
    """outside the limits: CBL_ERR_UNSUPPORTED (-3) and a workspace size of 0; a NULL input or a size outside its range: CBL_ERR_BAD_ARG (-1); a workspace one
    byte short: CBL_ERR_WORKSPACE (-2) — all before any launch; n2 == 0: a no-op"""
    n2, n1, c_up, c_skip, c_out, k = 40, 12, 8, 4, 12, 2
    case = O.make_case(n2, n1, c_up, c_skip, c_out, k, 0)
    coarse, skip, W, go, gamma, beta, inds = (case[key] for key in ("coarse", "skip", "W", "go", "gamma", "beta", "inds"))
    size = host.cbl_up_conv_workspace_bytes
    nbytes = size(ll(n2), ll(n1), c_up, c_skip, c_out)
    ws = aligned(np.zeros(nbytes, np.uint8))
    y, out, sm, si = nans(n2, c_out), nans(n2, c_out), nans(c_out), nans(c_out)

    def fwd(n2=n2, n1=n1, c_up=c_up, c_skip=c_skip, c_out=c_out, coarse=coarse, inds=inds, k=k, skip=skip, bn_mode=1, gamma=gamma, act=1, y=y, nbytes=nbytes,
            mm=None, ws=ws):
        return host.cbl_up_conv_forward(ll(n2), ll(n1), c_up, c_skip, c_out, P(coarse), P(inds), k, P(skip), P(W), None, bn_mode, P(gamma), P(beta), cf(1e-3),
                                        cf(0.98), P(mm), None, act, P(sm), P(si), P(y), P(out), P(ws), sz(nbytes), None)
    assert fwd(c_out=4097) == -3 and fwd(c_up=4000, c_skip=97) == -3
    assert size(ll(n2), ll(n1), c_up, c_skip, 4097) == 0 and size(ll(n2), ll(n1), 4000, 97, c_out) == 0 and size(ll(n2), ll(n1), 4000, 96, 4096) > 0
    assert size(ll(n2), ll(0), c_up, c_skip, c_out) == 0 and size(ll(-1), ll(n1), c_up, c_skip, c_out) == 0
    assert fwd(coarse=None) == -1 and fwd(inds=None) == -1 and fwd(skip=None) == -1 and fwd(gamma=None) == -1 and fwd(y=None) == -1
    assert fwd(bn_mode=3) == -1 and fwd(act=3) == -1 and fwd(c_up=0) == -1 and fwd(c_skip=0) == -1 and fwd(n1=0) == -1 and fwd(k=0) == -1 and fwd(n2=-1) == -1
    assert fwd(n2=1 << 30, k=2) == -1                                # n2 * k reaches 2^31
    assert fwd(mm=case["moving_mean"]) == -1                         # a moving mean without a moving variance
    assert fwd(bn_mode=2) == -1                                      # evaluation without moving statistics
    assert fwd(nbytes=nbytes - 1) == -2 and fwd(ws=None) == -2
    assert fwd(bn_mode=0, nbytes=nbytes - 1) == -2                   # coarse @ W_up lives in the workspace under every bn_mode
    assert fwd(n2=0) == 0
    assert not np.isfinite(out).any() and not np.isfinite(y).any() and not np.isfinite(sm).any()      # nothing was launched
    assert fwd() == 0
    inv_start, inv_src = first_column_table(inds, n1)
    g_c, g_s, g_W, g_g = nans(n1, c_up), nans(n2, c_skip), nans(c_up + c_skip, c_out), nans(c_out)

    def bwd(n2=n2, c_out=c_out, coarse=coarse, go=go, bn_mode=1, out=out, nbytes=nbytes, g_g=None, inv_start=inv_start, g_c=g_c, g_W=g_W):
        return host.cbl_up_conv_backward(ll(n2), ll(n1), c_up, c_skip, c_out, P(coarse), P(inds), k, P(skip), P(W), bn_mode, P(gamma), P(sm), P(si), 1, P(y),
                                         P(out), P(go), None, P(inv_start), P(inv_src), P(g_c), P(g_s), P(g_W), None, P(g_g), None, P(ws), sz(nbytes), None)
    assert bwd(c_out=4097) == -3
    assert bwd(coarse=None) == -1 and bwd(go=None) == -1 and bwd(out=None) == -1
    assert bwd(inv_start=None) == -1                                 # grad_coarse and grad_weights need the transposed table ...
    assert bwd(bn_mode=0, g_g=g_g) == -1                             # grad_gamma without a batch norm
    assert bwd(nbytes=nbytes - 1) == -2
    assert bwd(n2=0) == 0
    assert not any(np.isfinite(a).any() for a in (g_c, g_s, g_W, g_g))
    assert bwd(inv_start=None, g_c=None, g_W=None) == 0 and np.isfinite(g_s).all()      # ... grad_skip alone does not
    assert bwd(g_g=g_g) == 0 and all(np.isfinite(a).all() for a in (g_c, g_s, g_W, g_g))


def test_the_kernels_under_address_sanitizer():
    """the stand-alone program: the same translation units with -fsanitize=address,undefined, forward + backward over the shape edges, heap buffers of
    exactly their documented size"""
    r = run_sanitizer_program(sanitizer_program("up_conv", FILES, beside=True))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
