"""GPU: the segmentation head's decoder step (contrastboundary_amd/unary.up_conv over cbl_up_conv_*, csrc/up_conv.hip; tensorflow/models/heads/
seg_head.py:63-67) through the Python mirror with autograd, against the float64 restatement of the graph code in its direct form (tests/up_conv_oracle.py;
parity unpinned by execution — TF absent) within the 1e-4 contract.  The cases of tests/test_up_conv_host.py again on the device, and what only the mirror
has: a side stream, the module and its state_dict names, a CPU tensor raising, two calls giving the same bits, a captured and replayed graph of forward +
backward, and the composition conv1d_1x1(cat(nearest_upsample(coarse, inds), skip)) of the library's existing entries as a second reference.  Gradient cases
with relu or leaky_relu assert the oracle's no-flip precondition."""
import functools

import numpy as np
import pytest
import torch

from tests import up_conv_oracle as O

pytestmark = pytest.mark.gpu
LEAVES = (("grad_coarse", "coarse"), ("grad_skip", "skip"), ("grad_W", "W"), ("grad_biases", "b"), ("grad_gamma", "gamma"), ("grad_beta", "beta"))


def dev(a, off=0):
    """on the device; off = 4: the tensor starts 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.cuda()
    raw = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert raw.data_ptr() % 16 == 0
    view = raw[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def base_reference(bn, activation, bias):
    return O.reference(O.base_case(), bn, activation, bias)


def tensors(case, bn, bias, backward, off=0):
    g = lambda key, o=0: dev(case[key], o).requires_grad_(backward)
    t = dict(coarse=g("coarse", off), skip=g("skip", off), W=g("W", off), inds=dev(case["inds"]), b=g("biases") if bias else None, gamma=None, beta=None,
             mm=None, mv=None)
    if bn:
        t.update(gamma=g("gamma"), beta=g("beta"), mm=dev(case["moving_mean"]), mv=dev(case["moving_var"]))
    return t


def call(t, bn, activation, momentum=0.98):
    from contrastboundary_amd import unary
    return unary.up_conv(t["coarse"], t["inds"], t["skip"], t["W"], t["b"], t["gamma"], t["beta"], t["mm"], t["mv"], is_training=bn != "moving",
                         activation_fn=activation, bn_momentum=momentum)


def composed(t, bn, activation, momentum=0.98):
    """the same layer from the library's existing entries, with the upsampled and the concatenated tensor"""
    from contrastboundary_amd import local_aggregation, unary
    x = torch.cat([local_aggregation.nearest_upsample(t["coarse"], t["inds"]), t["skip"]], 1)
    return unary.conv1d_1x1(x, t["W"], t["b"], t["gamma"], t["beta"], t["mm"], t["mv"], is_training=bn != "moving", activation_fn=activation, bn_momentum=momentum)


def collect(t, out, bn, backward):
    res = dict(out=out.detach().cpu().numpy())
    if bn:
        res.update(moving_mean=t["mm"].cpu().numpy(), moving_var=t["mv"].cpu().numpy())
    if backward:
        for key, name in LEAVES:
            if t[name] is not None:
                res[key] = t[name].grad.cpu().numpy()
    res["raw"] = [v for k, v in sorted(res.items())]
    return res


def run(case, bn="batch", activation="relu", bias=True, backward=True, off=0, fn=call):
    """the mirror (or the composition) on the device -> dict(out, the gradients, moving_mean, moving_var, raw)"""
    t = tensors(case, bn, bias, backward, off)
    out = fn(t, bn, activation)
    if backward:
        out.backward(dev(case["go"], off))
    return collect(t, out, bn, backward)


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("activation", sorted(O.ACTIVATIONS))
def test_every_bn_mode_activation_and_bias(bn, activation):
    """the base shape and table: out, all gradients and the moving statistics; evaluation leaves the moving statistics alone"""
    case = O.base_case()
    for bias in (True, False):
        ref = base_reference(bn, activation, bias)
        O.assert_flip_free(ref, activation)
        res = run(case, bn, activation, bias)
        O.check(res, ref, bn, "%s %s bias %s" % (bn, activation, bias))
        assert (res["grad_coarse"][O.UNREFERENCED] == 0).all()
        # (that outputs are written and not accumulated is the host file's check: there every output is pre-filled with NaN; the mirror allocates its own)
        if bn == "moving":
            np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
            np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


@pytest.mark.parametrize("shape", O.EDGES + O.ODD)
def test_tile_edges_and_odd_widths(shape):
    case = O.make_case(*shape, 3)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch", "batch")
    O.check(run(case, None, "none"), O.reference(case, None, "none"), None, "bare")
    O.check(run(case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


def test_a_table_of_shadow_ids_only():
    case = O.make_case(*O.BASE, 4, kind="shadow")
    res = run(case, "batch", "none")
    O.check(res, O.reference(case, "batch", "none"), "batch")
    assert (res["grad_coarse"] == 0).all() and (res["grad_W"][:O.BASE[2]] == 0).all()


def test_bases_offset_by_4_bytes():
    case = O.base_case()
    for bn in O.BNS:
        ref = base_reference(bn, "leaky_relu", True)
        O.assert_flip_free(ref, "leaky_relu")
        O.check(run(case, bn, "leaky_relu", off=4), ref, bn, "offset %s" % bn)


@pytest.mark.parametrize("shape", O.CHUNKS)
def test_weight_gradient_chunks(shape):
    case = O.make_case(*shape, 5)
    for bn in ("batch", None):
        O.check(run(case, bn, "none"), O.reference(case, bn, "none"), bn, str(bn))


@pytest.mark.parametrize("shape", O.CAPS)
def test_more_tiles_and_trips_than_every_grid_cap(shape):
    case = O.make_case(*shape, 6)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch")


@pytest.mark.parametrize("shape", O.SPLITS)
def test_split_contraction_on_both_sides_of_its_rule(shape):
    case = O.make_case(*shape, 8)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch", "batch")
    O.check(run(case, None, "none"), O.reference(case, None, "none"), None, "bare")


@pytest.mark.parametrize("shape", O.EXTREMES)
def test_the_heads_extremes(shape):
    case = O.make_case(*shape, 7)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch")
    O.check(run(case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


@pytest.mark.parametrize("bn,activation", [("batch", "relu"), ("moving", "leaky_relu"), (None, "none")])
def test_the_mirror_equals_the_composition_of_the_existing_entries(bn, activation):
    """conv1d_1x1(cat(nearest_upsample(coarse, inds), skip)): outputs, all gradients and the moving statistics within `close` of each other (both are fp32;
    the composition takes the oracle's place, so the sums are held to `close` too) — at the base shape and at one with several chunks and shadow ids"""
    for case in (O.base_case(), O.multi_case()):
        O.assert_flip_free(O.reference(case, bn, activation, backward=False), activation)
        ours, theirs = run(case, bn, activation), run(case, bn, activation, fn=composed)
        assert sorted(ours) == sorted(theirs)
        for key in ours:
            if key == "raw":
                continue
            if key in ("grad_biases", "grad_gamma", "grad_beta"):
                ref = O.reference(case, bn, activation)
                O.close_sum(ours[key], theirs[key].astype(np.float64), ref[key[5:] + "_total"], key)
            else:
                O.close(ours[key], theirs[key].astype(np.float64), key)


def test_two_calls_give_identical_bits():
    case = O.multi_case()
    for bn, activation in (("batch", "relu"), ("moving", "leaky_relu"), (None, "none")):
        a = run(case, bn, activation)["raw"]
        b = run(case, bn, activation)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_on_a_side_stream():
    case = O.base_case()
    ref = base_reference("batch", "relu", True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = run(case)
    side.synchronize()
    O.check(res, ref, "batch")


def test_a_cpu_tensor_raises_and_so_do_bad_dtypes_and_shapes():
    from contrastboundary_amd import unary
    coarse, inds, skip, W = torch.zeros(5, 4), torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, 3), torch.zeros(7, 6)
    c = lambda t: t.cuda()
    with pytest.raises(TypeError):
        unary.up_conv(coarse, inds, skip, W)
    with pytest.raises(TypeError):
        unary.up_conv(c(coarse), inds, c(skip), c(W))
    with pytest.raises(TypeError):
        unary.up_conv(c(coarse), c(inds).long(), c(skip), c(W))
    with pytest.raises(TypeError):
        unary.up_conv(c(coarse).double(), c(inds), c(skip).double(), c(W).double())
    with pytest.raises(ValueError):
        unary.up_conv(c(coarse), c(inds), c(skip), torch.zeros(8, 6).cuda())          # c_up + c_skip != the weights' rows
    with pytest.raises(ValueError):
        unary.up_conv(c(coarse), c(inds)[:5].contiguous(), c(skip), c(W))             # the table's rows are not skip's
    with pytest.raises(ValueError):
        unary.up_conv(torch.zeros(0, 4).cuda(), c(inds), c(skip), c(W))               # no coarse row
    with pytest.raises(ValueError):
        unary.up_conv(c(coarse), c(inds), c(skip), c(W), gamma=torch.ones(6).cuda())
    with pytest.raises(ValueError):
        unary.up_conv(c(coarse), c(inds), c(skip), c(W), gamma=torch.ones(6).cuda(), beta=torch.zeros(6).cuda(), is_training=False)
    with pytest.raises(NotImplementedError):
        unary.up_conv(torch.zeros(5, 4000).cuda(), c(inds), torch.zeros(8, 97).cuda(), torch.zeros(4097, 6).cuda())
    assert unary.up_conv(c(coarse), torch.zeros(0, 2, dtype=torch.int32).cuda(), torch.zeros(0, 3).cuda(), c(W)).shape == (0, 6)


def test_no_fine_row_gives_zero_parameter_gradients():
    from contrastboundary_amd import unary
    coarse, W = torch.ones(5, 4).cuda().requires_grad_(True), torch.ones(7, 6).cuda().requires_grad_(True)
    out = unary.up_conv(coarse, torch.zeros(0, 2, dtype=torch.int32).cuda(), torch.zeros(0, 3).cuda(), W)
    out.sum().backward()
    assert out.shape == (0, 6) and (coarse.grad == 0).all() and (W.grad == 0).all()


def test_a_captured_graph_of_forward_and_backward_replays_the_eager_bits():
    """the transposed table of the first column is built in the warm-up step before the capture, and found again inside it"""
    case = O.multi_case()
    eager = run(case, "batch", "leaky_relu")
    t = tensors(case, "batch", True, True)
    go = dev(case["go"])
    leaves = [t[name] for _, name in LEAVES]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # a warm-up outside the capture: the library is loaded, the table is built and registered
        grads = torch.autograd.grad(call(t, "batch", "leaky_relu"), leaves, go)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(t, "batch", "leaky_relu")
        grads = torch.autograd.grad(out, leaves, go)
    for replay in range(2):
        t["mm"].copy_(dev(case["moving_mean"])); t["mv"].copy_(dev(case["moving_var"]))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(out=out, moving_mean=t["mm"], moving_var=t["mv"], **{key: g for (key, _), g in zip(LEAVES, grads)})
        for key, value in got.items():
            np.testing.assert_array_equal(value.detach().cpu().numpy().view(np.uint32), eager[key].view(np.uint32), err_msg="replay %d %s" % (replay, key))


def test_the_module():
    """variable names, shapes and tf_scopes() are those of Conv1d1x1(c_up + c_skip, out_fdim) — one `weights`, so a TF checkpoint loads unchanged; a round
    trip against the oracle in training and in evaluation"""
    from contrastboundary_amd import unary
    n2, n1, c_up, c_skip, c_out, k = O.BASE
    torch.manual_seed(0)
    m = unary.UpConv1d1x1(c_up, c_skip, c_out, with_bias=True, scope="up_conv0")
    plain = unary.Conv1d1x1(c_up + c_skip, c_out, with_bias=True, scope="up_conv0")
    assert list(m.state_dict()) == list(plain.state_dict()) == ["weights", "biases", "gamma", "beta", "moving_mean", "moving_variance"]
    assert {key: tuple(v.shape) for key, v in m.state_dict().items()} == {key: tuple(v.shape) for key, v in plain.state_dict().items()}
    assert tuple(m.weights.shape) == (c_up + c_skip, c_out)
    assert m.tf_scopes() == plain.tf_scopes() == dict(weights="up_conv0", biases="up_conv0", gamma="up_conv0/bn", beta="up_conv0/bn", moving_mean="up_conv0/bn",
                                                       moving_variance="up_conv0/bn")
    m.load_state_dict(plain.state_dict())                            # what loads into the plain layer loads into this one
    assert list(unary.UpConv1d1x1(c_up, c_skip, c_out, bn=False).state_dict()) == ["weights"]
    bound = (6.0 / (c_up + c_skip + c_out)) ** 0.5                   # xavier, uniform, over the whole variable
    w = unary.UpConv1d1x1(c_up, c_skip, c_out).weights.detach()
    assert float(w.abs().max()) <= bound and float(w.std()) > 0.4 * bound
    with pytest.raises(NotImplementedError):
        unary.UpConv1d1x1(4000, 97, c_out)
    with pytest.raises(NotImplementedError):
        unary.UpConv1d1x1(0, 36, c_out)
    m = m.cuda()
    m.activation_fn = "none"                                         # identity: no flip whatever the draw
    with torch.no_grad():
        m.gamma.uniform_(0.5, 1.5); m.moving_variance.uniform_(0.5, 1.5)
        m.beta.normal_(0.0, 0.3); m.biases.normal_(0.0, 0.3); m.moving_mean.normal_(0.0, 0.3)
    case = dict(O.base_case())
    for key, name in (("W", "weights"), ("biases", "biases"), ("gamma", "gamma"), ("beta", "beta"), ("moving_mean", "moving_mean"), ("moving_var", "moving_variance")):
        case[key] = getattr(m, name).detach().cpu().numpy().copy()
    ref = O.reference(case, "batch", "none")
    coarse, skip, inds = dev(case["coarse"]).requires_grad_(True), dev(case["skip"]).requires_grad_(True), dev(case["inds"])
    out = m(coarse, inds, skip)
    out.backward(dev(case["go"]))
    res = dict(out=out.detach().cpu().numpy(), grad_coarse=coarse.grad.cpu().numpy(), grad_skip=skip.grad.cpu().numpy(), grad_W=m.weights.grad.cpu().numpy(),
               grad_biases=m.biases.grad.cpu().numpy(), grad_gamma=m.gamma.grad.cpu().numpy(), grad_beta=m.beta.grad.cpu().numpy(),
               moving_mean=m.moving_mean.cpu().numpy(), moving_var=m.moving_variance.cpu().numpy())
    O.check(res, ref, "batch", "module")
    m.eval()                                                         # evaluation: the moving statistics, left alone
    before = [b.clone() for b in m.buffers()]
    case["moving_mean"], case["moving_var"] = m.moving_mean.cpu().numpy(), m.moving_variance.cpu().numpy()
    with torch.no_grad():
        out = m(dev(case["coarse"]), inds, dev(case["skip"]))
    O.close(out.cpu().numpy(), O.reference(case, "moving", "none", backward=False)["out"], "module in evaluation")
    for a, b in zip(before, m.buffers()):
        assert torch.equal(a, b)
