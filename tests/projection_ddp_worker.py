"""Worker of tests/test_projection_gpu.py::test_attach_reducer_covers_the_projection_gradients (a fresh process: it owns a process
group): a one-rank gloo group, zeng-ihome-proj, step.attach_reducer, one forward / backward.  Every trainable parameter's `.grad` must
lie inside the flat buffer of some reducer - the projection head's own buffer included - and a world-size-1 all-reduce (SUM) must leave
the gradients as they are."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out = sys.argv[1]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    from bihome_amd import configs, synth
    from bihome_amd.step import attach_reducer, build_model, build_optimizer
    from bihome_amd.weights import load_synthetic
    cfg = configs.get("zeng-ihome-proj")
    cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = 0.125
    model = build_model(cfg, "cuda")
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    opt, _ = build_optimizer(model, cfg["SOLVER"])
    red = attach_reducer(model)
    reducers = list(getattr(red, "reducers", [red]))
    B = 2
    d = synth.make_pairs(B, seed=77)
    data = {k: torch.tensor(d[k]).cuda() for k in ("patch_1", "patch_2", "delta")}
    data["choice_12"] = torch.randint(1, 128 * 128, (B, 128), generator=torch.Generator().manual_seed(5)).cuda()
    model.train()
    opt.zero_grad()
    loss, _, _ = model(data)
    loss.backward()
    torch.cuda.synchronize()
    spans = [(r.fg.flat.data_ptr(), r.fg.flat.data_ptr() + 4 * r.fg.flat.numel()) for r in reducers]
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    outside = [n for n, p in named if p.grad is None or not any(lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi
                                                                for lo, hi in spans)]
    proj = [(n, p) for n, p in named if "projection_head" in n]
    before = [p.grad.detach().clone() for _, p in named]
    red.allreduce()
    torch.cuda.synchronize()
    changed = [n for (n, p), b in zip(named, before) if not torch.equal(p.grad, b)]
    np.savez(out, loss=loss.item(), n_reducers=len(reducers), n_params=len(named), outside=np.array(outside, dtype=str),
             changed=np.array(changed, dtype=str), n_proj=len(proj), proj_grad_max=max(float(p.grad.abs().max()) for _, p in proj),
             deferred=np.array([bool(r.defer) for r in reducers]))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
