"""Write tests/golden/nguyen_orig_b4_{f32,f64}.npz: the photometric baseline (config/s-coco/nguyen-orig-lr-5e-3.yaml) on the
REFERENCE's own modules - src.backbones.ResNet34.Model (OneLine) + src.heads.PhotometricHead.Model + torch.nn.L1Loss (train.py:318-322),
with the kornia / torchvision / cv2 stand-ins of oracle/make_golden.py.  Runs only where the reference tree exists (never on the GPU box).

    python tools/make_golden_nguyen.py

An eval-mode predict_homography at the initial weights, then two Adam steps at the config's LR on one batch of
synth.make_pairs(4, seed=SEED, image=True) (the image is regenerated from the seed by the tests, not stored).  Recorded: per-step loss and MACE, delta_hat0, patch_hat0 subsampled
[..., ::8, ::8] and its (sum, |sum|, sum of squares), the gradient norms of the first and last two backbone parameters, and the eval
pair (delta_hat, H_hat)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF, csum, install_standins, sub, t  # noqa: E402

SEED = 23
BATCH = 4
KEYS = ("patch_1", "patch_2", "delta", "corners", "image_1")


def run(bb_cls, head_cls, cfg, dtype, batch=BATCH, seed=SEED, steps=2):
    from bihome_amd import synth
    from bihome_amd.weights import load_synthetic
    bb = bb_cls(**cfg["MODEL"]["BACKBONE"])
    head = head_cls(bb, **cfg["MODEL"]["HEAD"])
    load_synthetic(bb, seed=0)
    model = torch.nn.Sequential(bb, head).to(dtype)
    sol = cfg["SOLVER"]
    opt = torch.optim.Adam(model.parameters(), lr=sol["LR"], betas=(sol["MOMENTUM_1"], sol["MOMENTUM_2"]), weight_decay=0)
    loss_fn = getattr(torch.nn, sol["LOSS"])()
    d = synth.make_pairs(batch, seed=seed, image=True)
    out = {"loss": [], "mace": []}
    # inference first, at the initial weights and running statistics: after two steps at LR 5e-3 from random weights the eval-mode
    # outputs are ~1e8 px and the float32 / float64 runs differ by ~10 % - nothing to pin
    model.eval()
    with torch.no_grad():
        data = {k: t(d[k], dtype) for k in KEYS}
        dh, H = head.predict_homography(bb.predict_homography(data))          # eval.py:21-28
        out["eval_delta_hat"] = dh.double().numpy().copy()
        out["eval_H_hat"] = H.double().numpy().copy()
    for it in range(steps):
        model.train()
        data = {k: t(d[k], dtype) for k in KEYS}
        opt.zero_grad()
        ground_truth, network_output, delta_gt, delta_hat = model(data)
        loss = loss_fn(ground_truth, network_output)
        loss.backward()
        if it == 0:
            out["patch_hat0"] = sub(network_output)
            out["patch_hat0_csum"] = csum(network_output)
            out["delta_hat0"] = delta_hat.detach().double().numpy().copy()
            names = dict(bb.named_parameters())
            for name in list(names)[:2] + list(names)[-2:]:
                out["gradnorm/" + name] = np.float64(names[name].grad.double().norm().item())
        opt.step()
        out["loss"].append(loss.item())
        out["mace"].append(float(np.mean(np.linalg.norm((delta_gt - delta_hat).detach().double().numpy().reshape(-1, 2), axis=-1))))
    out["loss"], out["mace"] = np.array(out["loss"]), np.array(out["mace"])
    return out


def main():
    install_standins()
    import importlib
    ResNet34 = importlib.import_module("src.backbones.ResNet34")
    PhotometricHead = importlib.import_module("src.heads.PhotometricHead")
    for m in (ResNet34, PhotometricHead):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(REF)), m.__file__
    from bihome_amd import configs
    torch.set_num_threads(8)
    outdir = os.path.join(ROOT, "tests", "golden")
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        r = run(ResNet34.Model, PhotometricHead.Model, configs.get("nguyen-orig"), dtype)
        np.savez_compressed(os.path.join(outdir, "nguyen_orig_b4_%s.npz" % tag), **r)
        print("nguyen-orig", tag, "loss", r["loss"], "mace", r["mace"])


if __name__ == "__main__":
    main()
