"""GPU: the ConvNet's unary layer (contrastboundary_amd/unary.conv1d_1x1 over csrc/unary_layer.hip; tensorflow/models/basic_operators.py:195-241) through the
Python mirror with autograd, against the float64 restatement of the graph code (tests/unary_layer_oracle.py; parity unpinned by execution — TF absent) within
the 1e-4 contract.  The cases of tests/test_unary_layer_host.py again on the device, and what only the mirror has: a side stream, the module, a CPU tensor
raising, a captured and replayed graph of forward + backward.  Gradient cases with relu or leaky_relu assert the oracle's no-flip precondition."""
import functools

import numpy as np
import pytest
import torch

from tests import unary_layer_oracle as O

pytestmark = pytest.mark.gpu


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
def base_reference(bn, activation, shortcut, bias):
    return O.reference(O.base_case(), bn, activation, shortcut, bias)


def tensors(case, bn, shortcut, bias, backward, off=0):
    g = lambda key, o=0: dev(case[key], o).requires_grad_(backward)
    t = dict(x=g("x", off), W=g("W", off), b=g("biases") if bias else None, sc=g("shortcut", off) if shortcut else None, gamma=None, beta=None, mm=None, mv=None)
    if bn:
        t.update(gamma=g("gamma"), beta=g("beta"), mm=dev(case["moving_mean"]), mv=dev(case["moving_var"]))
    return t


def call(t, bn, activation, momentum=0.98):
    from contrastboundary_amd import unary
    return unary.conv1d_1x1(t["x"], t["W"], t["b"], t["gamma"], t["beta"], t["mm"], t["mv"], is_training=bn != "moving", activation_fn=activation,
                            bn_momentum=momentum, shortcut=t["sc"])


def collect(t, out, bn, backward):
    res = dict(out=out.detach().cpu().numpy())
    if bn:
        res.update(moving_mean=t["mm"].cpu().numpy(), moving_var=t["mv"].cpu().numpy())
    if backward:
        for key, name in (("grad_x", "x"), ("grad_W", "W"), ("grad_biases", "b"), ("grad_gamma", "gamma"), ("grad_beta", "beta"), ("grad_shortcut", "sc")):
            if t[name] is not None:
                res[key] = t[name].grad.cpu().numpy()
    res["raw"] = [v for k, v in sorted(res.items())]
    return res


def run(case, bn="batch", activation="relu", shortcut=True, bias=True, backward=True, off=0):
    """the mirror on the device -> dict(out, the gradients, moving_mean, moving_var, raw)"""
    t = tensors(case, bn, shortcut, bias, backward, off)
    out = call(t, bn, activation)
    if backward:
        out.backward(dev(case["go"], off))
    return collect(t, out, bn, backward)


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("activation", sorted(O.ACTIVATIONS))
def test_every_bn_mode_activation_shortcut_and_bias(bn, activation):
    """the base shape: out, all six gradients and the moving statistics; evaluation leaves the moving statistics alone"""
    case = O.base_case()
    for sc in (True, False):
        for bias in (True, False):
            ref = base_reference(bn, activation, sc, bias)
            O.assert_flip_free(ref, activation)
            res = run(case, bn, activation, sc, bias)
            O.check(res, ref, bn, "%s %s shortcut %s bias %s" % (bn, activation, sc, bias))
            # (that outputs are written and not accumulated is the host file's check: there every output is pre-filled with NaN; the mirror allocates its own)
            if bn == "moving":
                np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
                np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


@pytest.mark.parametrize("rows,c_in,c_out", O.EDGES)
def test_tile_edges(rows, c_in, c_out):
    case = O.make_case(rows, c_in, c_out, 3)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch", "batch")
    O.check(run(case, None, "none", shortcut=False), O.reference(case, None, "none", shortcut=False), None, "bare")
    O.check(run(case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


def test_a_base_pointer_offset_by_4_bytes_works():
    case = O.base_case()
    for bn in O.BNS:
        ref = base_reference(bn, "leaky_relu", True, True)
        O.assert_flip_free(ref, "leaky_relu")
        O.check(run(case, bn, "leaky_relu", off=4), ref, bn, "offset %s" % bn)


@pytest.mark.parametrize("rows,c_in,c_out", O.CHUNKS)
def test_weight_gradient_chunks(rows, c_in, c_out):
    case = O.make_case(rows, c_in, c_out, 5)
    for bn in ("batch", None):
        O.check(run(case, bn, "none"), O.reference(case, bn, "none"), bn, str(bn))


@pytest.mark.parametrize("rows,c_in,c_out", O.CAPS)
def test_more_tiles_and_trips_than_every_grid_cap(rows, c_in, c_out):
    """O.CAPS: the first shape walks past the cap of the row-tile kernels and of the column sums, the second past the cap of the elementwise passes"""
    case = O.make_case(rows, c_in, c_out, 6)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch")


@pytest.mark.parametrize("rows,c_in,c_out", O.EXTREMES)
def test_the_networks_extremes(rows, c_in, c_out):
    case = O.make_case(rows, c_in, c_out, 7)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch")
    O.check(run(case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")


def test_column_means_near_8():
    case = O.make_case(*O.BASE, O.SEED_MEAN_8, mean_8=True)
    for sc, bias in ((False, False), (True, True)):
        ref = O.reference(case, "batch", "relu", sc, bias)
        O.assert_flip_free(ref, "relu")
        O.check(run(case, "batch", "relu", sc, bias), ref, "batch")


def test_two_calls_give_identical_bits():
    case = O.make_case(1100, 36, 72, 0)
    for bn, activation in (("batch", "relu"), ("moving", "leaky_relu"), (None, "none")):
        a = run(case, bn, activation)["raw"]
        b = run(case, bn, activation)["raw"]
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_grad_biases_alone():
    """only the biases need a gradient: only the row of tiles that sums dy's columns is launched, and the bits are those of the full backward call"""
    for rows in (150, 1100):
        case = O.make_case(rows, 70, 72, 2)
        full = run(case, "batch", "none")
        t = tensors(case, "batch", True, True, False)
        t["b"].requires_grad_(True)
        call(t, "batch", "none").backward(dev(case["go"]))
        assert t["W"].grad is None and t["x"].grad is None
        np.testing.assert_array_equal(t["b"].grad.cpu().numpy().view(np.uint32), full["grad_biases"].view(np.uint32))


def test_on_a_side_stream():
    case = O.base_case()
    ref = base_reference("batch", "relu", True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = run(case)
    side.synchronize()
    O.check(res, ref, "batch")


def test_a_cpu_tensor_raises_and_so_do_bad_shapes():
    from contrastboundary_amd import unary
    x, W = torch.zeros(8, 4), torch.zeros(4, 6)
    with pytest.raises(TypeError):
        unary.conv1d_1x1(x, W)
    with pytest.raises(TypeError):
        unary.conv1d_1x1(x.cuda(), W)
    with pytest.raises(TypeError):
        unary.conv1d_1x1(x.cuda().double(), W.cuda().double())
    with pytest.raises(ValueError):
        unary.conv1d_1x1(x.cuda(), torch.zeros(5, 6).cuda())
    with pytest.raises(ValueError):
        unary.conv1d_1x1(x.cuda(), W.cuda(), gamma=torch.ones(6).cuda())
    with pytest.raises(ValueError):
        unary.conv1d_1x1(x.cuda(), W.cuda(), gamma=torch.ones(6).cuda(), beta=torch.zeros(6).cuda(), is_training=False)
    with pytest.raises(NotImplementedError):
        unary.conv1d_1x1(torch.zeros(2, 4097).cuda(), torch.zeros(4097, 6).cuda())
    assert unary.conv1d_1x1(torch.zeros(0, 4).cuda(), W.cuda()).shape == (0, 6)


def test_a_captured_graph_of_forward_and_backward_replays_the_eager_bits():
    case = O.make_case(1100, 36, 72, 1)
    eager = run(case, "batch", "leaky_relu")
    t = tensors(case, "batch", True, True, True)
    go = dev(case["go"])
    leaves = [t[k] for k in ("x", "W", "b", "gamma", "beta", "sc")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # a warm-up outside the capture: the library is loaded, autograd's buffers exist
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
        got = dict(out=out, grad_x=grads[0], grad_W=grads[1], grad_biases=grads[2], grad_gamma=grads[3], grad_beta=grads[4], grad_shortcut=grads[5],
                   moving_mean=t["mm"], moving_var=t["mv"])
        for key, value in got.items():
            np.testing.assert_array_equal(value.detach().cpu().numpy().view(np.uint32), eager[key].view(np.uint32), err_msg="replay %d %s" % (replay, key))


def test_the_module():
    """variable names, shapes, initialisers, tf_scopes(); a round trip against the oracle in training and in evaluation"""
    from contrastboundary_amd import unary
    torch.manual_seed(0)
    m = unary.Conv1d1x1(36, 72, with_bias=True, scope="conv1")
    assert list(m.state_dict()) == ["weights", "biases", "gamma", "beta", "moving_mean", "moving_variance"]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(weights=(36, 72), biases=(72,), gamma=(72,), beta=(72,), moving_mean=(72,),
                                                                           moving_variance=(72,))
    assert m.tf_scopes() == dict(weights="conv1", biases="conv1", gamma="conv1/bn", beta="conv1/bn", moving_mean="conv1/bn", moving_variance="conv1/bn")
    assert list(unary.Conv1d1x1(36, 72, bn=False).state_dict()) == ["weights"]
    assert unary.Conv1d1x1(36, 72, bn=False).tf_scopes() == dict(weights="")
    bound = (6.0 / (36 + 72)) ** 0.5                                 # xavier, uniform
    assert float(m.weights.detach().abs().max()) <= bound and float(m.weights.detach().std()) > 0.4 * bound
    assert (m.biases == 0).all() and (m.gamma == 1).all() and (m.beta == 0).all() and (m.moving_mean == 0).all() and (m.moving_variance == 1).all()
    f = unary.Conv1d1x1(360, 72, init="fan_in").weights.detach()
    std = (1.3 / 360) ** 0.5                                          # variance scaling, FAN_IN, truncated at two standard deviations
    assert float(f.abs().max()) <= 2 * std and 0.7 * std < float(f.std()) < std
    with pytest.raises(NotImplementedError):
        unary.Conv1d1x1(36, 72, init="other")
    with pytest.raises(NotImplementedError):
        unary.Conv1d1x1(36, 4097)
    # the module's own variables as the oracle's case (identity: no flip whatever the draw), moved off their initial values first
    m = m.cuda()
    m.activation_fn = "none"
    with torch.no_grad():
        m.gamma.uniform_(0.5, 1.5); m.moving_variance.uniform_(0.5, 1.5)
        m.beta.normal_(0.0, 0.3); m.biases.normal_(0.0, 0.3); m.moving_mean.normal_(0.0, 0.3)
    case = O.base_case()
    for key, name in (("W", "weights"), ("biases", "biases"), ("gamma", "gamma"), ("beta", "beta"), ("moving_mean", "moving_mean"), ("moving_var", "moving_variance")):
        case[key] = getattr(m, name).detach().cpu().numpy().copy()
    ref = O.reference(case, "batch", "none")
    x, sc = dev(case["x"]).requires_grad_(True), dev(case["shortcut"]).requires_grad_(True)
    out = m(x, sc)
    out.backward(dev(case["go"]))
    res = dict(out=out.detach().cpu().numpy(), grad_x=x.grad.cpu().numpy(), grad_shortcut=sc.grad.cpu().numpy(), grad_W=m.weights.grad.cpu().numpy(),
               grad_biases=m.biases.grad.cpu().numpy(), grad_gamma=m.gamma.grad.cpu().numpy(), grad_beta=m.beta.grad.cpu().numpy(),
               moving_mean=m.moving_mean.cpu().numpy(), moving_var=m.moving_variance.cpu().numpy())
    O.check(res, ref, "batch", "module")
    m.eval()                                                         # evaluation: the moving statistics, left alone
    before = [b.clone() for b in m.buffers()]
    case["moving_mean"], case["moving_var"] = m.moving_mean.cpu().numpy(), m.moving_variance.cpu().numpy()
    with torch.no_grad():
        out = m(dev(case["x"]), dev(case["shortcut"]))
    O.close(out.cpu().numpy(), O.reference(case, "moving", "none", backward=False)["out"], "module in evaluation")
    for a, b in zip(before, m.buffers()):
        assert torch.equal(a, b)
