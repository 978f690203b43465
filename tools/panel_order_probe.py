"""Same-process A/B of the bf16 chain learner's update chunk (forward_loss() + backward_fused()) with its internal activations
and dZ row-major, with the dZ in panel order, and with both in panel order (include/trajopt_grpo_hip.h TG_LAYOUT_PANEL): HIP-event
time per launch of the three kernel families, the configurations interleaved `--passes` times so that drift shows as spread.
Prints one JSON line per net.
usage: python tools/panel_order_probe.py [--rows N] [--hidden H] [--layers L] [--iters K] [--passes P] [--configs a,b] [--nets 4,1]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trajopt_grpo_amd as tg
from trajopt_grpo_amd import mlp as M

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 22)
ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--layers", type=int, default=5)
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--configs", default="row_major,dz_panel,all_panel")
ap.add_argument("--nets", default="4,1", help="output widths: 4 = the actor (clipped surrogate), 1 = the critic (squared error)")
a_ = ap.parse_args()
rows, H, nh = a_.rows, a_.hidden, a_.layers
dev = torch.device("cuda", 0)
CONFIGS = {"row_major": (False, False), "dz_panel": (True, False), "all_panel": (True, True)}
CONFIGS = {k: CONFIGS[k] for k in a_.configs.split(",")}

for A, kind in [(int(w), 0 if int(w) > 1 else 1) for w in a_.nets.split(",")]:
    torch.manual_seed(A)
    net = tg.NeuralNetwork(20, A, (H,) * nh, "ReLU").to(dev)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    mlp = M.GemmMLP(net, torch.bfloat16)
    xp = mlp.prepare_input(torch.randn(rows, 20, device=dev))
    act = torch.randn(rows, A, device=dev)
    lpo = (-0.5 * torch.rand(rows, device=dev) - 1.0).contiguous()
    adv, ret = torch.randn(rows, device=dev), torch.randn(rows, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)

    def chunk():
        if kind == 0:
            mlp.forward_loss(xp, 0, act=act, logp_old=lpo, adv=adv, norm=[0.1, 1.3], var=torch.full((A,), 0.3), epsilon=0.2,
                             surr_coef=-1.0 / rows, kl_coef=0.0, sums_out=sums)
        else:
            mlp.forward_loss(xp, 1, ret=ret, norm=[-0.2, 0.7], critic_coef=0.5 / rows, sums_out=sums)
        mlp.backward_fused()

    out = {"rows": rows, "hidden": H, "layers": nh, "outputs": A, "iters": a_.iters, "us_per_launch": {}, "tb_per_s": {}, "bytes_per_row": {}}
    for _ in range(a_.passes):
        for name, (panel, head) in CONFIGS.items():
            mlp.panel_order, M.PANEL_ORDER_HEAD_PASS, mlp.panel_mixed = panel, head, True
            for _ in range(2):
                chunk()
            mlp.fwd_events, mlp.dx_events, mlp.dw_events = [], [], []
            for _ in range(a_.iters):
                chunk()
            torch.cuda.synchronize()
            for fam, evs in (("fwd", mlp.fwd_events), ("bwd", mlp.dx_events), ("dw", mlp.dw_events)):
                us = sorted(1e3 * e0.elapsed_time(e1) for e0, e1, *_ in evs)
                med = us[len(us) // 2]
                out["bytes_per_row"][fam] = evs[0][3]
                out["us_per_launch"].setdefault(f"{fam}/{name}", []).append(round(med, 1))
                out["tb_per_s"].setdefault(f"{fam}/{name}", []).append(round(evs[0][2] * evs[0][3] / med / 1e6, 3))
            mlp.fwd_events = mlp.dx_events = mlp.dw_events = None
    print(json.dumps(out), flush=True)
    del mlp, xp, act, lpo, adv, ret
    torch.cuda.empty_cache()
