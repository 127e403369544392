"""run-to-run spread of a 4-step eager training trajectory on the golden 8192-point scene (python tools/traj_determinism.py [fused|split|plain] [deterministic]);
a trailing `deterministic` runs under contrastboundary_amd.set_deterministic(True): expected spread 0"""
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_gpu_model import build, CASES  # noqa: E402
from contrastboundary_amd import blocks  # noqa: E402

args = sys.argv[1:]
det = bool(args) and args[-1] == "deterministic"
if det:
    import contrastboundary_amd
    contrastboundary_amd.set_deterministic(True)
    args = args[:-1]
mode = args[0] if args else "fused"
M, model, crit, g = build(CASES[0])
model = model.cuda().train()
for m in model.modules():
    if isinstance(m, blocks.PointTransformerLayer):
        m.fused = {"fused": True, "split": "split", "plain": False}[mode]
inputs = {"points": torch.from_numpy(g("xyz")).cuda(), "features": torch.from_numpy(g("feat")).cuda(), "offset": torch.from_numpy(g("offset")).cuda()}
target = torch.from_numpy(g("target")).cuda()
inputs2 = {"points": (inputs["points"] * torch.tensor([-1.0, 1.0, 1.0], device="cuda")).contiguous(), "features": inputs["features"].flip(0).contiguous(),
           "offset": inputs["offset"].clone()}
target2 = target.roll(17)
batches = [(inputs, target), (inputs2, target2), (inputs, target), (inputs2, target2)]
runs = []
for r in range(4):
    twin = copy.deepcopy(model)
    opt = torch.optim.SGD(twin.parameters(), lr=0.002, momentum=0.9)
    traj = []
    for b_in, b_tg in batches:
        opt.zero_grad(set_to_none=True)
        _, _, loss, _ = M.forward_and_loss(twin, crit, b_in, b_tg)
        loss.sum().backward()
        opt.step()
        traj.append(loss.detach().cpu().numpy().astype(np.float64))
    runs.append(np.stack(traj))
ref = runs[0]
print("mode", mode, "deterministic" if det else "")
for s in range(4):
    dev = max(float(np.max(np.abs(r[s] - ref[s]) / np.maximum(np.abs(ref[s]), 1e-12))) for r in runs[1:])
    print("step %d  loss %s  max relative spread over 3 reruns %.2e" % (s, np.array2string(ref[s], precision=4), dev))
