"""The trainable projection head (WITH_PROJECTION_HEAD) at B = 64 on one MI355X:
  1. the training step of zeng-ihome-proj / zeng-ihome-cos-proj / detone-bihome-proj (head [[64,128],[128,64]]) against the same config
     without the projection;
  2. the projection + L2 normalisation forward and the anchor-adjoint + normalisation-adjoint + projection backward on the stacked
     [2B,32,32,64] unwarped maps and the [B,32,32,64] warped map, against the torch formulation (F.linear, relu, division by norm;
     autograd for the adjoint).
Prints one JSON line per measurement; `--out FILE` also writes them to a JSON file.

    python tools/projection_head_bench.py [--batch 64] [--steps 30] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def step_times(B, steps):
    from bihome_amd import configs, synth
    from bihome_amd.step import build_model, build_optimizer, train_step
    from bihome_amd.weights import load_synthetic
    d = synth.make_pairs(B, seed=42)
    ch = [torch.randint(1, 128 * 128, (B, 128), generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2)]
    out = []
    for base, margin in (("zeng-ihome", 0.125), ("zeng-ihome-cos", 0.015625), ("detone-bihome", None)):
        ms = {}
        for name in (base, base + "-proj"):
            cfg = configs.get(name)
            if margin is not None:
                cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = margin
            model = build_model(cfg)
            load_synthetic(model[0], 0)
            load_synthetic(model[1].auxiliary_resnet, 0)
            opt, sched = build_optimizer(model, cfg["SOLVER"])
            data = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
            data["choice_12"], data["choice_21"] = ch
            ms[name] = timed(lambda: train_step(model, data, opt, sched), steps)
            del model, opt
            torch.cuda.empty_cache()
        out.append({"what": "step", "config": base, "batch": B, "ms_per_step": round(ms[base], 3),
                    "ms_per_step_proj": round(ms[base + "-proj"], 3), "added_ms": round(ms[base + "-proj"] - ms[base], 3)})
    return out


def path_times(B, steps):
    """One-line L1 path of the head from the extractor's features to the loss: forward = project both maps + normalise + loss;
    backward = loss and anchor adjoints + normalisation adjoints + the projection's two backward walks (weight gradients, input
    gradient of the warped map only).  (A NetFunction node can be walked back once: the backward is timed together with its forward.)"""
    from bihome_amd import kernels as K
    from bihome_amd.heads import PerceptualHead
    from bihome_amd.weights import load_synthetic
    widths = [(64, 128), (128, 64)]
    ph = load_synthetic(PerceptualHead._ProjectionHead(widths, "f32"), 0).cuda().train()
    g = torch.Generator().manual_seed(0)
    feat, featw = torch.randn(2 * B, 32, 32, 64, generator=g).cuda(), torch.randn(B, 32, 32, 64, generator=g).cuda()
    cov = torch.rand(B, 32, 32, generator=g).cuda()
    gl = torch.ones(1, device="cuda")
    state = {}

    def hip_fwd():
        fwl = featw.detach().requires_grad_(True)
        pa, pw = ph(feat), ph(fwl)
        (ya, ia), (yw, iw) = K.l2norm_fwd(pa.detach()), K.l2norm_fwd(pw.detach())
        loss, T, nd, _ = K.oneline_loss_fwd(ya[:B], ya[B:], yw, cov, 0.125)
        state.update(fwl=fwl, pa=pa, pw=pw, ya=ya, ia=ia, yw=yw, iw=iw, T=T, nd=nd)

    def hip_fwd_bwd():
        hip_fwd()
        s = state
        gfw, _ = K.oneline_loss_bwd(gl, s["ya"][B:], s["yw"], cov, s["T"], s["nd"])
        ga = torch.empty_like(s["ya"])
        K.oneline_anchor_bwd(gl, s["ya"][:B], s["ya"][B:], s["yw"], cov, s["T"], s["nd"], out=ga)
        torch.autograd.backward([s["pa"]], [K.l2norm_bwd(ga, s["ya"], s["ia"])])
        torch.autograd.grad(s["pw"], s["fwl"], K.l2norm_bwd(gfw, s["yw"], s["iw"]))

    layers = [(ph[i].weight.detach().clone().requires_grad_(True), ph[i].bias.detach().clone().requires_grad_(True)) for i in (0, 2)]

    def proj(x):
        return F.linear(torch.relu(F.linear(x, *layers[0])), *layers[1])

    def torch_fwd():
        fwl = featw.detach().requires_grad_(True)
        ya, yw = proj(feat), proj(fwl)
        ya, yw = ya / torch.norm(ya, p=2, dim=-1, keepdim=True), yw / torch.norm(yw, p=2, dim=-1, keepdim=True)
        t = (yw - ya[B:]).abs().sum(-1) - (ya[:B] - ya[B:]).abs().sum(-1) + 0.125
        den = cov.sum((-1, -2))
        state.update(tfwl=fwl, tloss=((cov * t.clamp_min(0)).sum((-1, -2)) / torch.max(den, torch.ones_like(den))).sum())

    def torch_fwd_bwd():
        torch_fwd()
        torch.autograd.grad(state["tloss"], [state["tfwl"]] + [t for pair in layers for t in pair])

    out = []
    for what, fn in (("hip forward (project x2 + l2norm x2 + loss)", hip_fwd),
                     ("hip forward + backward (+ loss and anchor adjoints + l2norm x2 + project x2)", hip_fwd_bwd),
                     ("torch forward (F.linear, relu, / norm, loss in torch)", torch_fwd), ("torch forward + backward (autograd)", torch_fwd_bwd)):
        out.append({"what": "path", "leg": what, "batch": B, "ms": round(timed(fn, steps), 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rows = path_times(a.batch, a.steps) + step_times(a.batch, a.steps)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
