"""GPU: pool_bn (contrastboundary_amd/unary.pool_bn over csrc/pool_bn.hip: TF batch norm + activation behind every local aggregation) through the Python mirror
with autograd, against the float64 restatement in the direct form (tests/pool_bn_oracle.py; parity unpinned by execution — TF absent): every entry within
1e-4 of its column's scale.  The cases of tests/test_pool_bn_host.py again on the device, and what only the mirror has: a side stream, the module in train()
and eval(), a CPU tensor raising, a captured and replayed graph of forward + backward.  Gradient cases with relu or leaky_relu assert the oracle's no-flip
precondition."""
import functools

import numpy as np
import pytest
import torch

from tests import pool_bn_oracle as O

pytestmark = pytest.mark.gpu


def dev(a, place="aligned"):
    """on the device.  'odd': rows 1.. of a (rows + 1, C) tensor (with C odd the base is not 16-byte aligned); 'off4': 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if place == "aligned":
        return t.cuda()
    if place == "odd":
        big = torch.zeros(t.shape[0] + 1, t.shape[1], dtype=t.dtype, device="cuda")
        view = big[1:]
    else:
        raw = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
        view = raw[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def tensors(case, bn, backward, place="aligned"):
    t = dict(x=dev(case["x"], place).requires_grad_(backward), gamma=None, beta=None, mm=None, mv=None)
    if bn:
        t.update(gamma=dev(case["gamma"]).requires_grad_(backward), beta=dev(case["beta"]).requires_grad_(backward), mm=dev(case["moving_mean"]),
                 mv=dev(case["moving_var"]))
    return t


def call(t, bn, activation, momentum=0.98, eps=1e-3):
    from contrastboundary_amd import unary
    return unary.pool_bn(t["x"], t["gamma"], t["beta"], t["mm"], t["mv"], is_training=bn != "moving", activation_fn=activation, bn_momentum=momentum,
                         bn_eps=eps)


def collect(t, out, bn, backward):
    res = dict(out=out.detach().cpu().numpy())
    if bn:
        res.update(moving_mean=t["mm"].cpu().numpy(), moving_var=t["mv"].cpu().numpy())
    if backward:
        res["grad_x"] = t["x"].grad.cpu().numpy()
        if bn:
            res.update(grad_gamma=t["gamma"].grad.cpu().numpy(), grad_beta=t["beta"].grad.cpu().numpy())
    res["raw"] = [v for k, v in sorted(res.items())]
    return res


def run(case, bn="batch", activation="relu", backward=True, place="aligned", momentum=0.98, eps=1e-3):
    """the mirror on the device -> dict(out, the gradients, moving_mean, moving_var, raw)"""
    t = tensors(case, bn, backward, place)
    out = call(t, bn, activation, momentum, eps)
    if backward:
        out.backward(dev(case["go"], place))
    return collect(t, out, bn, backward)


@functools.lru_cache(maxsize=None)
def base_reference(bn, activation):
    return O.reference(O.make_case(*O.BASE, O.SEED), bn, activation)


@pytest.mark.parametrize("bn", O.BNS)
@pytest.mark.parametrize("activation", sorted(O.ACTIVATIONS))
def test_every_bn_mode_and_activation(bn, activation):
    case = O.make_case(*O.BASE, O.SEED)
    ref = base_reference(bn, activation)
    O.assert_flip_free(ref, activation)
    res = run(case, bn, activation)
    O.check(res, ref, bn, "%s %s" % (bn, activation))
    if bn == "moving":
        np.testing.assert_array_equal(res["moving_mean"], case["moving_mean"])
        np.testing.assert_array_equal(res["moving_var"], case["moving_var"])


@pytest.mark.parametrize("rows,C", O.SHAPES + O.CAP_SHAPES)
def test_shapes(rows, C):
    """O.SHAPES and O.CAP_SHAPES (the host file's): both sides of the single-launch rule, every width class, more rows than the grid cap"""
    case = O.make_case(rows, C, 3)
    O.check(run(case, "batch", "none"), O.reference(case, "batch", "none"), "batch", "batch")
    O.check(run(case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "relu")
    O.check(run(case, "moving", "leaky_relu", backward=False), O.reference(case, "moving", "leaky_relu", backward=False), "moving", "moving")


def test_an_unaligned_base():
    for rows, C, place in ((150, 3, "odd"), (1100, 7, "odd"), (150, 72, "off4")):
        case = O.make_case(rows, C, 4)
        for bn in O.BNS:
            O.check(run(case, bn, "none", place=place), O.reference(case, bn, "none"), bn, "unaligned %s" % bn)


@pytest.mark.parametrize("rows", [300, 3000])                        # the single launch, the chunked launches
def test_ill_conditioned_columns(rows):
    """|mean| / std up to 1e4 and an exactly constant column (tests/test_pool_bn_host.py derives the bound and shows that the uncentred formula fails it)"""
    case = O.ill_case(rows, 24, 11)
    ref = O.reference(case, "batch", "none")
    res = run(case, "batch", "none")
    O.check(res, ref, "batch", "ill-conditioned %d" % rows)
    hard = [c for c in range(24) if c % 4 == 3]
    err = np.abs(res["out"].astype(np.float64) - ref["out"])[:, hard].max(0)
    print("ill-conditioned, rows %d: worst |out - ref| / (eps32 |mean| invstd |gamma|) on the 1e4 columns: %.3f" % (rows, float((err / ref["floors"]["out"][hard]).max())))
    assert (err <= ref["floors"]["out"][hard]).all()
    O.check(run(case, "batch", "relu", backward=False), O.reference(case, "batch", "relu", backward=False), "batch", "ill-conditioned relu")
    np.testing.assert_array_equal(res["out"][:, 5], np.full(rows, case["beta"][5], np.float32))


def test_moving_statistics_one_row_and_no_row():
    case = O.make_case(200, 12, 1)
    O.check(run(case, "batch", "none", momentum=0.9, eps=1e-5), O.reference(case, "batch", "none", momentum=0.9, eps=1e-5), "batch", "momentum 0.9")
    one = O.make_case(1, 12, 2)
    res = run(one, "batch", "none")
    np.testing.assert_array_equal(res["out"][0], one["beta"])        # variance 0: xhat = 0
    np.testing.assert_allclose(res["moving_var"], one["moving_var"] * np.float32(0.98), rtol=1e-6)
    none = {k: (v[:0] if v.ndim == 2 else v) for k, v in one.items()}
    res = run(none, "batch", "relu")
    assert res["out"].shape == (0, 12) and res["grad_x"].shape == (0, 12) and not res["grad_gamma"].any() and not res["grad_beta"].any()
    np.testing.assert_array_equal(res["moving_mean"], one["moving_mean"]); np.testing.assert_array_equal(res["moving_var"], one["moving_var"])


def test_two_calls_give_identical_bits():
    for rows in (300, 1100):
        case = O.make_case(rows, 72, 0)
        for bn, activation in (("batch", "relu"), ("moving", "leaky_relu"), (None, "none")):
            a = run(case, bn, activation)["raw"]
            b = run(case, bn, activation)["raw"]
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_on_a_side_stream():
    case = O.make_case(*O.BASE, O.SEED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = run(case)
    side.synchronize()
    O.check(res, base_reference("batch", "relu"), "batch", "side stream")


def test_a_cpu_tensor_raises_and_so_do_bad_arguments():
    from contrastboundary_amd import unary
    x, g = torch.zeros(8, 4), torch.ones(4)
    with pytest.raises(TypeError):
        unary.pool_bn(x, g, g)
    with pytest.raises(TypeError):
        unary.pool_bn(x.cuda(), g, g.cuda())
    with pytest.raises(TypeError):
        unary.pool_bn(x.cuda().double())
    with pytest.raises(TypeError):
        unary.pool_bn(torch.zeros(8, 8).cuda()[:, :4])               # not contiguous
    with pytest.raises(ValueError):
        unary.pool_bn(torch.zeros(8).cuda())
    with pytest.raises(ValueError):
        unary.pool_bn(x.cuda(), gamma=g.cuda())
    with pytest.raises(ValueError):
        unary.pool_bn(x.cuda(), g.cuda(), torch.zeros(5).cuda())
    with pytest.raises(ValueError):
        unary.pool_bn(x.cuda(), g.cuda(), g.cuda(), moving_mean=g.cuda())
    with pytest.raises(ValueError):
        unary.pool_bn(x.cuda(), moving_mean=g.cuda(), moving_variance=g.cuda())
    with pytest.raises(ValueError):
        unary.pool_bn(x.cuda(), g.cuda(), g.cuda(), is_training=False)
    with pytest.raises(NotImplementedError):
        unary.pool_bn(torch.zeros(2, 4097).cuda())
    assert unary.pool_bn(torch.zeros(0, 4).cuda(), g.cuda(), g.cuda()).shape == (0, 4)


def test_a_captured_graph_of_forward_and_backward_replays_the_eager_bits():
    for rows in (300, 1100):                                         # the single launch, the chunked launches
        case = O.make_case(rows, 72, 1)
        eager = run(case, "batch", "leaky_relu")
        t = tensors(case, "batch", True)
        go = dev(case["go"])
        leaves = [t[k] for k in ("x", "gamma", "beta")]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                # a warm-up outside the capture: the library is loaded, autograd's buffers exist
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
            got = dict(out=out, grad_x=grads[0], grad_gamma=grads[1], grad_beta=grads[2], moving_mean=t["mm"], moving_var=t["mv"])
            for key, value in got.items():
                np.testing.assert_array_equal(value.detach().cpu().numpy().view(np.uint32), eager[key].view(np.uint32), err_msg="replay %d %s" % (replay, key))


def test_the_module():
    """variable names, shapes, initial values, tf_scopes(); train() against the oracle with the buffers updated, eval() with the buffers left alone"""
    from contrastboundary_amd import unary
    m = unary.PoolBN(72)
    assert list(m.state_dict()) == ["gamma", "beta", "moving_mean", "moving_variance"]
    assert m.tf_scopes() == dict(gamma="pool_bn", beta="pool_bn", moving_mean="pool_bn", moving_variance="pool_bn")
    assert unary.PoolBN(72, scope="bn").tf_scopes()["gamma"] == "bn"
    assert list(unary.PoolBN(72, bn=False).state_dict()) == [] and unary.PoolBN(72, bn=False).tf_scopes() == {}
    assert (m.gamma == 1).all() and (m.beta == 0).all() and (m.moving_mean == 0).all() and (m.moving_variance == 1).all()
    with pytest.raises(NotImplementedError):
        unary.PoolBN(4097)
    m = m.cuda()
    m.activation_fn = "none"
    with torch.no_grad():
        m.gamma.uniform_(0.5, 1.5); m.moving_variance.uniform_(0.5, 1.5); m.beta.normal_(0.0, 0.3); m.moving_mean.normal_(0.0, 0.3)
    case = O.make_case(*O.BASE, O.SEED)
    for key, name in (("gamma", "gamma"), ("beta", "beta"), ("moving_mean", "moving_mean"), ("moving_var", "moving_variance")):
        case[key] = getattr(m, name).detach().cpu().numpy().copy()
    ref = O.reference(case, "batch", "none")
    x = dev(case["x"]).requires_grad_(True)
    out = m(x)
    out.backward(dev(case["go"]))
    res = dict(out=out.detach().cpu().numpy(), grad_x=x.grad.cpu().numpy(), grad_gamma=m.gamma.grad.cpu().numpy(), grad_beta=m.beta.grad.cpu().numpy(),
               moving_mean=m.moving_mean.cpu().numpy(), moving_var=m.moving_variance.cpu().numpy())
    O.check(res, ref, "batch", "module")
    m.eval()
    before = [b.clone() for b in m.buffers()]
    case["moving_mean"], case["moving_var"] = m.moving_mean.cpu().numpy(), m.moving_variance.cpu().numpy()
    with torch.no_grad():
        out = m(dev(case["x"]))
    O.check(dict(out=out.cpu().numpy()), O.reference(case, "moving", "none", backward=False), "moving", "module in evaluation")
    for a, b in zip(before, m.buffers()):
        assert torch.equal(a, b)
    # bn=False: the activation alone
    out = unary.PoolBN(72, activation_fn="leaky_relu", bn=False).cuda()(dev(case["x"]))
    np.testing.assert_array_equal(out.cpu().numpy(), np.where(case["x"] > 0, case["x"], np.float32(0.2) * case["x"]))
