"""GPU: the CBL head on feature rows of any width (csrc/cbl_pairs.hip, the chunked pair kernels) — against the reference's own ContrastHead run on
the stage outputs ('f_out', 32 ... 512 wide) and the class logits ('logits', 13 wide) (tests/golden/cbl_wide_pytorch.npz, gen_cbl_wide_goldens.py), against
the oracle over the width / neighbour-count grid of tests/test_cbl_wide_host.py, and for the properties the training step relies on: the gather route is
deterministic, a captured graph replays what eager computes, and the widths of the original kernels give the same bits before and after a wide call."""
import os

import numpy as np
import pytest
import torch

from oracle import cbl_oracle as C
from tests import test_cbl_wide_host as H

pytestmark = pytest.mark.gpu
W = np.load(os.path.join(os.path.dirname(__file__), "golden", "cbl_wide_pytorch.npz"))
TOL = 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Cfg(dict):
    __getattr__ = dict.__getitem__


def head_config(ftype):
    return Cfg(nsample=[int(v) for v in W["nsample"]], nstride=[int(v) for v in W["nstride"]], num_classes=13, num_layers=5, voxel_size=0.04, base_fdim=32,
               contrast=Cfg(stage="Ua", contrast="softnn", ftype=ftype, sample="label", pos="cnt", dist="l2", temperature=float(W["temperature"]),
                            weight="w.1"))


@pytest.mark.parametrize("ftype", ["f_out", "logits"])
def test_contrast_head_on_stage_outputs_and_logits_matches_reference(ftype):
    from contrastboundary_amd.heads import ContrastHead
    cfg = head_config(ftype)
    head = ContrastHead(cfg.contrast, cfg)
    up = []
    for i in range(5):
        f = dev(W[f"{ftype}/stage{i}/features_x32"].astype(np.float32) / 32).requires_grad_(True)
        up.append({"p_out": dev(W[f"{ftype}/stage{i}/p"]), "offset": dev(W[f"{ftype}/stage{i}/offset"]), ftype: f})
    sl = {"inputs": None, "up": up, "down": up}
    losses = head(None, dev(W[f"{ftype}/target"]), sl)
    assert len(losses) == 5
    torch.stack(losses).sum().backward()
    for i in range(5):
        want = float(W[f"{ftype}/stage{i}/loss"])
        assert abs(losses[i].item() - want) <= TOL * max(1.0, abs(want)), (i, losses[i].item(), want)
        g, rg = up[i][ftype].grad.cpu().numpy(), W[f"{ftype}/stage{i}/grad"]
        assert g.shape == rg.shape
        np.testing.assert_allclose(g, rg, rtol=TOL, atol=TOL * max(float(np.abs(rg).max()), 1e-30))
    assert float(W[f"{ftype}/stage4/loss"]) > 0                           # the widest stage takes part


def device_pairs(feat, labels, samples, flags, T, weight, ncls=0, kl=0.0, roles=None, valid=None):
    """the C entries on device tensors: forward, then the gather over the transposed table and the atomic scatter -> loss, mask, grads"""
    import ctypes
    from contrastboundary_amd import _lib, pointops
    m, d = feat.shape
    nsample = samples.shape[1]
    L, ci, cf, st = _lib.lib(), ctypes.c_int, ctypes.c_float, _lib.stream_of(feat)
    e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=feat.device)
    per_point, mask, stats, loss, coef, own = e(m), e(m, dt=torch.int32), e(2), e(1), e(m, nsample), e(m, d)
    _lib.check(L.cbl_contrast_pairs_forward_samples(ci(m), ci(m), ci(flags), ci(nsample), ci(d), _lib.ptr(feat), _lib.ptr(labels), ci(ncls), cf(kl),
                                                    _lib.ptr(samples), _lib.ptr(roles), _lib.ptr(valid), _lib.ptr(None), cf(T), cf(weight), _lib.ptr(per_point),
                                                    _lib.ptr(mask), _lib.ptr(stats), _lib.ptr(loss), _lib.ptr(coef), _lib.ptr(own), st), "forward")
    one = torch.ones(1, dtype=torch.float32, device=feat.device)
    order, inv_start, inv_src = pointops.neighbor_transpose(samples, m)
    gg, ga = e(m, d), e(m, d)
    _lib.check(L.cbl_contrast_pairs_backward(ci(m), ci(nsample), ci(d), _lib.ptr(feat), _lib.ptr(coef), _lib.ptr(own), _lib.ptr(order), _lib.ptr(inv_start),
                                             _lib.ptr(inv_src), _lib.ptr(stats), _lib.ptr(one), cf(weight), _lib.ptr(gg), st), "backward")
    _lib.check(L.cbl_contrast_pairs_backward_atomic(ci(m), ci(m), ci(nsample), ci(d), _lib.ptr(feat), _lib.ptr(coef), _lib.ptr(own), _lib.ptr(samples),
                                                    _lib.ptr(stats), _lib.ptr(one), cf(weight), _lib.ptr(ga), st), "backward_atomic")
    torch.cuda.synchronize()
    return float(loss.item()), mask.cpu().numpy(), gg.cpu().numpy(), ga.cpu().numpy()


def device_points(d):
    return 3000 if d <= 256 else 600


@pytest.mark.parametrize("d,nsample", H.GRID)
def test_point_contrast_any_width_vs_oracle(d, nsample):
    from contrastboundary_amd import heads
    n, T, weight = device_points(d), 0.7, 0.1
    _, feat, lab, idx = H.scene(n, nsample, d, seed=d + nsample)
    for contrast in ("softnn", "nce"):
        f = dev(feat).requires_grad_(True)
        loss, mask = heads.point_contrast(f, dev(lab.astype(np.int64)), dev(idx), temperature=T, weight=weight, return_mask=True, contrast=contrast)
        loss.backward()
        rloss, rgrad, rmask = C.point_contrast(np.array(feat), np.eye(13, dtype=np.float32)[lab], idx, temperature=T, weight=weight, contrast=contrast)
        H.check(loss.item(), mask.cpu().numpy(), (f.grad.cpu().numpy(),), rloss, rgrad, rmask)
        _, _, gg, ga = device_pairs(dev(feat), dev(lab), dev(idx), 4 if contrast == "nce" else 0, T, weight)
        H.check(loss.item(), mask.cpu().numpy(), (gg, ga), rloss, rgrad, rmask)


@pytest.mark.parametrize("d,nsample", H.GRID)
def test_tf_contrast_any_width_vs_oracle(d, nsample):
    from contrastboundary_amd import heads
    n, T, weight = device_points(d), 0.8, 0.1
    xyz, feat, lab, _ = H.scene(n, nsample, d, seed=2 * d + nsample)
    lab = lab.copy(); lab[::17] = -1
    nb = H.radius_columns(xyz, nsample, seed=d)
    for contrast, margin, atomic in (("softnn", None, False), ("softnn", None, True), ("nce", None, False), ("softnn", "S", False)):
        f = dev(feat).requires_grad_(True)
        loss, mask = heads.tf_contrast(f, dev(lab), dev(nb), temperature=T, weight=weight, return_mask=True, contrast=contrast, margin=margin,
                                       atomic_scatter=atomic)
        loss.backward()
        rloss, rgrad, rmask = C.tf_contrast(np.array(feat), lab, nb, temperature=T, weight=weight, contrast=contrast, separate=margin == "S")
        H.check(loss.item(), mask.cpu().numpy(), (f.grad.cpu().numpy(),), rloss, rgrad, rmask)


@pytest.mark.parametrize("d", [3, 13, 72, 512, 2304])
def test_tf_sample_roles_and_labelkl_any_width(d):
    from contrastboundary_amd import heads
    n, k, T, weight = device_points(d), 17, 0.9, 0.1
    xyz, feat, lab, _ = H.scene(n, k, d, seed=d + 101)
    nbr = H.radius_columns(xyz, k, seed=d + 5)
    rng = np.random.default_rng(d)
    r1, r2 = rng.integers(0, n, (n, 6)).astype(np.int32), rng.integers(0, n, (n, 3)).astype(np.int32)
    r2[:, 0] = np.minimum(nbr[:, 2], n - 1)
    sample = "nn2-label-rand6-rand3R"
    soft = (0.8 * np.eye(5)[lab % 5] + 0.2 * rng.dirichlet(np.full(5, 0.5), n)).astype(np.float32)
    for kl in (None, 0.4):
        f = dev(feat).requires_grad_(True)
        labels = dev(lab) if kl is None else dev(soft)
        loss, mask = heads.tf_contrast(f, labels, dev(nbr), temperature=T, weight=weight, return_mask=True, kl_threshold=kl, sample=sample,
                                       rand_idx=[dev(r1), dev(r2)])
        loss.backward()
        rloss, rgrad, rmask = C.tf_contrast(np.array(feat), lab if kl is None else soft, nbr, temperature=T, weight=weight, kl_threshold=kl, sample=sample,
                                            rand_idx=[r1, r2])
        assert rmask.any()
        H.check(loss.item(), mask.cpu().numpy(), (f.grad.cpu().numpy(),), rloss, rgrad, rmask)


@pytest.mark.parametrize("d", [13, 256, 2304])
def test_gather_route_is_bit_identical_run_to_run(d):
    from contrastboundary_amd import heads
    n = device_points(d)
    _, feat, lab, idx = H.scene(n, 36, d, seed=d)
    runs = []
    for _ in range(2):
        f = dev(feat).requires_grad_(True)
        loss = heads.point_contrast(f, dev(lab), dev(idx), 0.7, 0.1)
        loss.backward()
        runs.append((loss.detach().cpu().numpy().copy(), f.grad.cpu().numpy().copy()))
    assert runs[0][1].any()
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))


def test_graph_replay_of_a_wide_stage_equals_eager():
    """d = 256 forward + backward captured in one graph (the transposed table built by the warm-up, found in the registry during capture)"""
    from contrastboundary_amd import heads
    n, d = 640, 256
    _, feat, lab, idx = H.scene(n, 24, d, seed=4)
    f, lab_d, idx_d = dev(feat).requires_grad_(True), dev(lab), dev(idx)
    out = {}

    def step():
        loss = heads.point_contrast(f, lab_d, idx_d, 0.7, 0.1)
        (g,) = torch.autograd.grad(loss, f)
        out["loss"], out["grad"] = loss.detach(), g

    step()
    eager = (out["loss"].clone(), out["grad"].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    out["grad"].zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert eager[1].abs().max().item() > 0
    assert torch.equal(out["loss"], eager[0]) and torch.equal(out["grad"], eager[1])


def test_original_widths_unchanged_around_a_wide_call():
    """d = 32 / 64 run the original kernels: the same bits before and after a d = 512 and a d = 13 call in the same process"""
    from contrastboundary_amd import heads

    def run(d, seed):
        _, feat, lab, idx = H.scene(4000 if d <= 64 else 600, 36, d, seed=seed)
        f = dev(feat).requires_grad_(True)
        loss = heads.point_contrast(f, dev(lab), dev(idx), 0.7, 0.1)
        loss.backward()
        return loss.detach().cpu().numpy().view(np.uint32).copy(), f.grad.cpu().numpy().view(np.uint32).copy()

    before = [run(32, 1), run(64, 2)]
    run(512, 3); run(13, 4)
    after = [run(32, 1), run(64, 2)]
    for (l0, g0), (l1, g1) in zip(before, after):
        assert np.array_equal(l0, l1) and np.array_equal(g0, g1)


@pytest.mark.parametrize("ftype", ["f_out", "logits"])
def test_training_step_with_a_wide_contrast_feature(ftype):
    """a reference-format config contrasting the stage outputs or the logits (contrast.ftype, multi.ftype) builds its criterion and trains a step"""
    from contrastboundary_amd import pointtransformer_seg as M
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_pytorch.npz"))
    case = sorted({k.split("/")[0] for k in G.files})[0]
    g = lambda key: G[f"{case}/{key}"]
    cfg = M.Config({"base_fdim": 32, "nsample": [36, 24, 24, 24, 24], "nstride": [4, 4, 4, 4], "ignore_label": 255, "voxel_size": 0.04,
                    "contrast": {"stage": "Ua", "contrast": "softnn", "ftype": ftype, "sample": "label", "pos": "cnt", "dist": "l2",
                                 "temperature": 1, "weight": "w.1"},
                    "multi": {"stage": "Ua", "ftype": "logits" if ftype == "logits" else "latent", "combine": "concat"}})
    torch.manual_seed(0)
    model = M.pointtransformer_seg_repro(c=6, k=13, config=cfg).cuda().train()
    crit = M.Loss(cfg)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    inputs = {"points": dev(g("xyz")), "features": dev(g("feat")), "offset": dev(g("offset"))}
    _, stage_list, loss, _ = M.forward_and_loss(model, crit, inputs, dev(g("target")))
    assert loss.shape == (6,) and torch.isfinite(loss).all()
    widths = [st[ftype].shape[1] for st in stage_list["up"]]
    assert widths == ([32, 64, 128, 256, 512] if ftype == "f_out" else [13] * 5)
    assert (loss[1:] > 0).any()
    loss.sum().backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
    opt.step()
    torch.cuda.synchronize()
