"""GPU: the TF-side update (csrc/tf_update.hip through its C entries, and contrastboundary_amd.tf_train over them) against the float64 restatement of the
reference's update (tests/tf_update_oracle.py; parity unpinned by execution — TF absent) within the bounds derived there.  The cases of
tests/test_tf_update_host.py again on the device, and what only the device and the Python layer have: weight_loss under autograd, TFMomentum's views, idle
parameters, state_dict, a captured and replayed clip_and_step() following set_lr, and three training steps of a two-layer Conv1d1x1 stack with
cross_entropy against the float64 oracles (tests/unary_layer_oracle.py for the layers) under the same update rule, on a seed without relu flips."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import tf_update_oracle as O
from tests import unary_layer_oracle as U

pytestmark = pytest.mark.gpu


def put(a, off=0):
    """on the device in a buffer of exactly a.size (+ off) elements; off: the base lies that many elements behind a 256-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    raw = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    assert raw.data_ptr() % 16 == 0
    view = raw[off:]
    view.copy_(t)
    return view


@pytest.fixture(scope="module")
def drv():
    from contrastboundary_amd import _lib
    return O.Driver(_lib.lib(), put, lambda x: x.cpu().numpy(), lambda x: ctypes.c_void_p(x.data_ptr()))


@pytest.fixture(scope="module")
def edge(drv):
    case = O.edge_case()
    return case, drv.layout(case)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\ntf_update: largest error / bound on the device:", {k: "%.3f" % v for k, v in sorted(O.ratios.items())})


def test_every_mode_on_the_edge_buffer(drv):
    O.check_all_modes(drv, O.edge_case(), "edge buffer")


@pytest.mark.parametrize("size", O.EDGE_SIZES)
def test_every_mode_on_one_segment(drv, size):
    O.check_all_modes(drv, O.make_case([size], 100 + size, wd=[0.05]), "S = 1, %d" % size)


@pytest.mark.parametrize("off", [(0, 1, 0), (0, 0, 2), (3, 3, 3)])
def test_buffers_that_disagree_modulo_16_bytes(drv, edge, off):
    case, lay = edge
    for mode, fold in ((O.CLIP | O.STEP, 1), (O.CLIP, 0), (O.STEP, 0)):
        O.check_update(drv, case, lay, mode, fold, off=off, what="bases at %s" % (off,))


def test_weight_loss_value_terms_gradient_and_unread_segments(drv, edge):
    O.check_weight_loss(drv, *edge)
    case = O.make_case([O.CHUNK + 1], 3, wd=[0.3])
    O.check_weight_loss(drv, case, drv.layout(case))


def test_pinned_gradient_norms(drv, edge):
    O.check_pinned_norms(drv, *edge)


def test_idle_segments_keep_value_and_momentum(drv, edge):
    O.check_inactive(drv, *edge, idle={0, 7, 9})


def test_two_calls_give_the_same_bits(drv, edge):
    O.check_deterministic(drv, *edge)


def test_one_chunk_more_than_the_launch_cap(drv):
    """4096 waves at most per launch: 4097 chunks (34 MB a buffer) make the last chunk a wave's second trip"""
    case = O.make_case([3, O.CAP_CHUNKS * O.CHUNK - O.CHUNK + 1], 11, wd=[0.0, 0.02])
    lay = drv.layout(case)
    assert lay["nc"].value == O.CAP_CHUNKS + 1
    O.check_update(drv, case, lay, O.CLIP | O.STEP, 1, clip_norm=100.0, what="past the cap")
    O.check_weight_loss(drv, case, lay)


# ---------------------------------------------------------------------------------------------- tf_train
def make_params(sizes, seed):
    rng = np.random.default_rng(seed)
    return [torch.nn.Parameter(torch.from_numpy(rng.normal(size=s).astype(np.float32)).cuda()) for s in sizes]


SHAPES = [(3, 5), (65,), (O.CHUNK + 1,), (7,), (2, O.CHUNK)]
COEF = [0.05, 0.0, 0.01, 0.0, 0.5]


def flat_case(params, grads, accum=None):
    """the oracle's view of a parameter list: flat arrays and begins"""
    sizes = [int(np.prod(p.shape)) for p in params]
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = lambda xs: np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in xs])
    return dict(total=int(begin[-1]), S=len(sizes), begin=begin, wd=np.asarray(COEF, np.float32), params=flat(params), grads=flat(grads),
                accum=flat(accum) if accum is not None else np.zeros(int(begin[-1]), np.float32))


def test_momentum_views_weight_loss_and_steps_against_the_oracle():
    from contrastboundary_amd import tf_train
    params = make_params(SHAPES, 1)
    before = [p.detach().cpu().numpy().copy() for p in params]
    opt = tf_train.TFMomentum(params, lr=O.LR, momentum=O.MOMENTUM, grad_norm=O.CLIP_NORM, coefficients=COEF)
    assert all(p.data_ptr() == opt.flat_param.data_ptr() + 4 * int(b) for p, b in zip(params, opt.layout.begin_host))
    assert all(np.array_equal(p.detach().cpu().numpy(), b) for p, b in zip(params, before)) and all(p.grad is g for p, g in zip(params, opt.grad_views))
    # loss = a linear form of the parameters + the weight loss: the gradient is the form's coefficients + wd w
    rng = np.random.default_rng(2)
    coeffs = [rng.normal(size=s).astype(np.float32) for s in SHAPES]
    opt.zero_grad()
    wl, terms = opt.weight_loss(return_terms=True)
    loss = sum((p * torch.from_numpy(c).cuda()).sum() for p, c in zip(params, coeffs)) + 0.75 * wl
    loss.backward()
    case = flat_case(before, coeffs)
    eloss, eterms = O.weight_loss(case["params"], case["begin"], case["wd"])
    O.relative(wl.item(), eloss, "weight loss")
    O.relative(terms.cpu().numpy(), eterms, "weight loss terms")
    egrad = O.f64(case["grads"]) + O.weight_loss_grad(case["params"], case["begin"], case["wd"], O.f32(0.75))
    O.within(opt.flat_grad.cpu().numpy(), egrad, np.abs(O.f64(case["grads"])) + np.abs(egrad), "weight loss gradient")
    case["grads"] = opt.flat_grad.cpu().numpy().copy()
    norms = opt.clip().cpu().numpy().copy()
    gp, enorms = O.clip(case["params"], case["grads"], case["begin"], case["wd"], O.f32(O.CLIP_NORM), False)
    O.relative(norms, enorms, "norms")
    opt.step()
    ew, ea = O.momentum_step(case["params"], case["accum"], gp, O.f32(O.LR), O.f32(O.MOMENTUM))
    _, _, _, _, sc = O.expected_update(case, O.CLIP | O.STEP, 0, O.CLIP_NORM, 1.0, O.LR, O.MOMENTUM)
    O.within(opt.flat_accum.cpu().numpy(), ea, sc["a"], "momentum")
    O.within(torch.cat([p.detach().reshape(-1) for p in params]).cpu().numpy(), ew, sc["w"], "updated parameter")
    # fold_decay: the same step from the form's gradient alone, in one call
    params2 = make_params(SHAPES, 1)
    opt2 = tf_train.TFMomentum(params2, lr=O.LR, momentum=O.MOMENTUM, grad_norm=O.CLIP_NORM, coefficients=COEF, fold_decay=True)
    opt2.zero_grad()
    sum((p * torch.from_numpy(c).cuda()).sum() for p, c in zip(params2, coeffs)).backward()
    opt2.clip_and_step()
    case2 = flat_case(before, coeffs)
    ew2, _, ea2, _, sc2 = O.expected_update(case2, O.CLIP | O.STEP, 1, O.CLIP_NORM, 1.0, O.LR, O.MOMENTUM)
    O.within(opt2.flat_accum.cpu().numpy(), ea2, sc2["a"], "momentum")
    O.within(opt2.flat_param.cpu().numpy(), ew2, sc2["w"], "updated parameter")


def test_a_parameter_without_a_gradient_keeps_value_and_momentum():
    from contrastboundary_amd import tf_train
    params = make_params(SHAPES, 3)
    opt = tf_train.TFMomentum(params, lr=0.1, grad_norm=1.0)
    opt.flat_accum.normal_()
    state = opt.state_dict()
    opt.zero_grad()
    (params[0].sum() * 2 + (params[2] ** 2).sum()).backward()        # parameters 1, 3 and 4 receive nothing
    w0, a0 = opt.flat_param.clone(), opt.flat_accum.clone()
    opt.clip_and_step()
    for i, (p, a) in enumerate(zip(params, opt.accum_views)):
        b, e = int(opt.layout.begin_host[i]), int(opt.layout.begin_host[i + 1])
        same = torch.equal(opt.flat_param[b:e], w0[b:e]) and torch.equal(opt.flat_accum[b:e], a0[b:e])
        assert same == (i in (1, 3, 4)), i
    # a foreign zero_grad(set_to_none=True) drops the views: the next backward pass's gradients are taken in, the views come back
    for p in params:
        p.grad = None
    (params[1] * 3).sum().backward()
    assert params[1].grad is not opt.grad_views[1]
    w1 = opt.flat_param.clone()
    opt.clip_and_step()
    assert all(p.grad is g for p, g in zip(params, opt.grad_views)) and torch.allclose(opt.grad_views[1], torch.full((65,), 65 ** -0.5, device="cuda"), rtol=1e-6, atol=0)
    b, e = int(opt.layout.begin_host[1]), int(opt.layout.begin_host[2])
    assert not torch.equal(opt.flat_param[b:e], w1[b:e]) and torch.equal(opt.flat_param[:b], w1[:b]) and torch.equal(opt.flat_param[e:], w1[e:])
    # state_dict keeps the momentum by name
    other = tf_train.TFMomentum(make_params(SHAPES, 4), lr=0.5)
    other.load_state_dict(state)
    assert torch.equal(other.flat_accum, a0) and other.state_dict()["lr"] == 0.1 and sorted(state["momentum_buffers"]) == sorted(opt.names)
    with pytest.raises(KeyError):
        other.load_state_dict({"momentum_buffers": {"param_0": state["momentum_buffers"]["param_0"]}})


def test_captured_clip_and_step_follows_set_lr_bit_for_bit():
    from contrastboundary_amd import tf_train
    rng = np.random.default_rng(5)
    grads = [torch.from_numpy(rng.normal(size=s).astype(np.float32)).cuda() * 3 for s in SHAPES]

    def fresh():
        opt = tf_train.TFMomentum(make_params(SHAPES, 6), lr=0.01, grad_norm=O.CLIP_NORM, coefficients=COEF, fold_decay=True)
        opt.zero_grad()
        sum((p * g).sum() for p, g in zip(opt.params, grads)).backward()
        return opt

    def refill(opt):                                                 # clip_and_step leaves the clipped gradients behind: the same raw gradients again
        for v, g in zip(opt.grad_views, grads):
            v.copy_(g)

    eager = fresh()
    eager.clip_and_step()
    refill(eager); eager.set_lr(0.003); eager.clip_and_step()
    refill(eager); eager.set_lr(0.02); eager.clip_and_step()
    captured = fresh()
    captured.clip_and_step()                                         # warm-up: the set of parameters with a gradient is on the device
    refill(captured)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.clip_and_step()
    # (the capture ran nothing: the state is the one after the warm-up step)
    captured.set_lr(0.003); graph.replay()
    refill(captured); captured.set_lr(0.02); graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.flat_param, eager.flat_param) and torch.equal(captured.flat_accum, eager.flat_accum)
    assert torch.equal(captured.flat_grad, eager.flat_grad) and torch.equal(captured.norms, eager.norms)


# ---------------------------------------------------------------------------------------------- three training steps
ROWS, C_IN, C_MID, CLASSES, STEPS, WD = 150, 36, 24, 13, 3, 0.05
TRAIN_LR, TRAIN_CLIP = 0.05, 0.3                                       # a clip norm the two weight gradients exceed and the others do not


def train_inputs(seed):
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f32(rng.normal(size=(ROWS, C_IN))), labels=rng.integers(0, CLASSES, ROWS).astype(np.int64),
                W1=f32(rng.normal(size=(C_IN, C_MID)) / np.sqrt(C_IN)), gamma=f32(rng.uniform(0.5, 1.5, C_MID)), beta=f32(rng.normal(0, 0.3, C_MID)),
                W2=f32(rng.normal(size=(C_MID, CLASSES)) / np.sqrt(C_MID)), b2=f32(rng.normal(0, 0.5, CLASSES)))


def oracle_training(inp):
    """three steps in float64: the layers by tests/unary_layer_oracle.reference (forward, then backward under the upstream gradient), the mean cross entropy
    and the weight loss by hand, the update by tests/tf_update_oracle.  -> (losses, final variables, smallest |pre-activation| met, norms of the last step)"""
    v = {k: O.f64(inp[k]) for k in ("W1", "gamma", "beta", "W2", "b2")}
    acc = {k: np.zeros_like(a) for k, a in v.items()}
    mm, mv = np.zeros(C_MID), np.ones(C_MID)
    zeros = lambda *s: np.zeros(s)
    losses, min_z = [], np.inf
    for _ in range(STEPS):
        c1 = dict(x=O.f64(inp["x"]), W=v["W1"], biases=zeros(C_MID), shortcut=zeros(ROWS, C_MID), gamma=v["gamma"], beta=v["beta"], moving_mean=mm, moving_var=mv,
                  go=zeros(ROWS, C_MID))
        f1 = U.reference(c1, "batch", "relu", False, False, backward=False)
        min_z = min(min_z, f1["min_abs_z"])
        c2 = dict(x=f1["out"], W=v["W2"], biases=v["b2"], shortcut=zeros(ROWS, CLASSES), gamma=zeros(CLASSES), beta=zeros(CLASSES), moving_mean=zeros(CLASSES),
                  moving_var=zeros(CLASSES), go=zeros(ROWS, CLASSES))
        logits = U.reference(c2, None, "none", False, True, backward=False)["out"]
        z = logits - logits.max(1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(1, keepdims=True))
        ce = -logp[np.arange(ROWS), inp["labels"]].mean()
        wl = WD * 0.5 * (np.sum(v["W1"] ** 2) + np.sum(v["W2"] ** 2))
        losses.append(ce + wl)
        dlogits = np.exp(logp)
        dlogits[np.arange(ROWS), inp["labels"]] -= 1
        c2["go"] = dlogits / ROWS
        r2 = U.reference(c2, None, "none", False, True)
        c1["go"] = r2["grad_x"]
        r1 = U.reference(c1, "batch", "relu", False, False)
        mm, mv = r1["moving_mean"], r1["moving_var"]
        g = dict(W1=r1["grad_W"] + WD * v["W1"], gamma=r1["grad_gamma"], beta=r1["grad_beta"], W2=r2["grad_W"] + WD * v["W2"], b2=r2["grad_biases"])
        norms = {}
        for k in v:
            gp, norms[k] = O.clip_by_norm(g[k], TRAIN_CLIP)
            v[k], acc[k] = O.momentum_step(v[k], acc[k], gp, TRAIN_LR, O.MOMENTUM)
    return losses, v, min_z, norms


@functools.lru_cache(maxsize=None)
def training_reference():
    """the first seed on which no pre-activation of the relu layer comes within 1e-5 of zero in any of the three steps (the project's flip-free practice)"""
    for seed in range(16):
        inp = train_inputs(seed)
        ref = oracle_training(inp)
        if ref[2] >= 1e-5:
            return inp, ref
    raise AssertionError("no flip-free seed")


@pytest.mark.parametrize("fold", [False, True])
def test_three_training_steps_of_a_two_layer_stack(fold):
    from contrastboundary_amd import tf_train
    from contrastboundary_amd.pointtransformer_seg import cross_entropy
    from contrastboundary_amd.unary import Conv1d1x1
    inp, (elosses, ev, min_z, enorms) = training_reference()
    assert min_z >= 1e-5
    l1 = Conv1d1x1(C_IN, C_MID, scope="l1").cuda()
    l2 = Conv1d1x1(C_MID, CLASSES, with_bias=True, activation_fn=None, bn=False, scope="l2").cuda()
    with torch.no_grad():
        for p, k in ((l1.weights, "W1"), (l1.gamma, "gamma"), (l1.beta, "beta"), (l2.weights, "W2"), (l2.biases, "b2")):
            p.copy_(torch.from_numpy(inp[k]))
    opt = tf_train.TFMomentum([l1, l2], lr=TRAIN_LR, momentum=O.MOMENTUM, grad_norm=TRAIN_CLIP, weight_decay=WD, fold_decay=fold)
    assert opt.names == ["l1/weights", "l1/bn/gamma", "l1/bn/beta", "l2/weights", "l2/biases"] and opt.coefficients == [WD, 0.0, 0.0, WD, 0.0]
    x, labels = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["labels"]).cuda()
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        ce = cross_entropy(l2(l1(x)), labels)
        wl = opt.weight_loss()
        (ce if fold else ce + wl).backward()
        losses.append(float(ce.detach()) + float(wl.detach()))
        opt.clip_and_step()
    U.close(np.array(losses), np.array(elosses), "losses")
    got_norms = opt.norms.cpu().numpy()
    U.close(got_norms, np.array([enorms[k] for k in ("W1", "gamma", "beta", "W2", "b2")]), "norms of the last step")
    assert got_norms.max() > TRAIN_CLIP > got_norms.min(), got_norms                    # both sides of the clip are met
    for p, k in ((l1.weights, "W1"), (l1.gamma, "gamma"), (l1.beta, "beta"), (l2.weights, "W2"), (l2.biases, "b2")):
        U.close(p.detach().cpu().numpy(), ev[k], "final " + k)
        # the step itself against the start: an update that did nothing would pass `close` on a small learning rate
        assert np.abs(p.detach().cpu().numpy() - inp[k]).max() > 1e-3
