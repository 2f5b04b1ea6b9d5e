"""Write the fixtures of the trainable projection head (AuxiliaryResnet WITH_PROJECTION_HEAD, PerceptualHead.py:41-48,69-74) by running
the REFERENCE's own Rethinking.py, ResNet34.py and PerceptualHead.py through the stand-ins of oracle/make_golden.py.  Runs only where
the reference tree exists (never on the GPU box).

    python tools/make_golden_projection.py

tests/golden/zeng_ihome_proj_b4_{f32,f64}.npz          zeng-ihome + projection, one hypothesis, two Adam steps on synth.make_pairs(4, seed=23)
tests/golden/zeng_ihome_cos_proj_n4_b4_{f32,f64}.npz   zeng-ihome-cos + projection, RANSAC_HYPOTHESIS_NO = 4, POINTS_PER_HYPOTHESIS = 16
tests/golden/detone_bihome_proj_b4_{f32,f64}.npz       detone-bihome + projection (string margin: no hinge), two Adam steps, same batch
The head is [[64, 96], [96, 32]]: a hidden width that is no power of two, 32 channels into the loss.  Each file holds what
oracle.make_golden.run_bihome_variant / run_detone_steps record, the chosen `margin` (inf: the double-line string margin), the
`active_share`, the head's state-dict key names and shapes (`sd_keys`, `sd_shapes`), and - float64 files only - the step-0 maps that
restate the loss, computed HERE in float64 from what the reference's AuxiliaryResnet.forward returned (projected, NOT yet normalised)
and the warped all-ones masks (Model._warp):
  one-line      l1, l3, w [B*n,32,32] (upstream's names: l1 = d(f1w, f2), l3 = d(f1, f2) on the L2-normalised maps; cosine: 1 - c) and
                scores0 [B*n] for n = 4
  double-line   M1, M2, w1, w2 [B,32,32] and the two homographies H1, H2 [B,3,3] of the mu term
plus, for tests of the projection itself, the extractor's features IN FRONT of the projection at every 8th pixel (`pre_f1`, `pre_f2`,
`pre_f1w`[, `pre_f2w`], NHWC [.,4,4,64]; the input of the first Linear, caught by a forward pre-hook).
The loss restated from the maps is asserted equal to the reference's step-0 loss to 1e-9 relative.

One-line margins are chosen HERE as tools/make_golden_loss_variants.py chooses them: the first value of the ladder 2^(-k/2) at which
the share of active hinge terms at step 0 (over the pixels with w > 0) lies in [0.2, 0.8]."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden_loss_variants import LADDER, Record, cos, first_of_ladder, pooled, save  # noqa: E402
from oracle.make_golden import REF, install_standins, run_bihome_variant, run_detone_steps  # noqa: E402

SEED, BATCH, N_HYP, N_PTS = 23, 4, 4, 16
WIDTHS = [[64, 96], [96, 32]]
SUB = 8


class RecordFirstLinearInputs:
    """Keep (a float64 copy of) what enters the projection head's first Linear, call by call: the extractor's NHWC features."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        def hook(module, args):
            if isinstance(module, torch.nn.Linear) and (module.in_features, module.out_features) == tuple(WIDTHS[0]) and args[0].dim() == 4:
                self.calls.append(args[0].detach().double().clone())
        self._handle = torch.nn.modules.module.register_module_forward_pre_hook(hook)
        return self

    def __exit__(self, *exc):
        self._handle.remove()


def l2n(x):
    """PerceptualHead.py:470-479 on NCHW maps: x / torch.norm(x, p=2, dim=1)."""
    return x / torch.norm(x, p=2, dim=1).unsqueeze(dim=1)


def oneline_maps(feats, warps, cosine):
    f1, f2, f1w = (l2n(c[0]) for c in feats[:3])
    w = pooled(warps[1][0], f1.shape[-1])
    if cosine:
        return dict(l1=1 - cos(f1w, f2), l3=1 - cos(f1, f2), w=w)
    return dict(l1=(f1w - f2).abs().sum(1), l3=(f1 - f2).abs().sum(1), w=w)


def oneline_loss(m, margin, scores=None):
    t = (m["l1"] - m["l3"] + margin).clamp_min(0)
    per = (m["w"] * t).sum((1, 2)) / m["w"].sum((1, 2)).clamp_min(1.0)
    return float((per * (1.0 if scores is None else scores)).sum())


def oneline_share(m, margin):
    return float(((m["l1"] - m["l3"] + margin) > 0)[m["w"] > 0].double().mean())


def bihome_maps(feats, warps):
    f1, f2, f1w, f2w = (c[0] for c in feats[:4])             # (not normalised: PerceptualHead.py:545-557 is commented out)
    l3 = (f1 - f2).abs()
    size = f1.shape[-1]
    return dict(M1=((f1w - f2).abs() - l3).sum(1), M2=((f2w - f1).abs() - l3).sum(1), w1=pooled(warps[1][0], size),
                w2=pooled(warps[3][0], size), H1=warps[0][1], H2=warps[2][1])


def bihome_loss(m, mu):
    ln = [float(((m["w%d" % i] * m["M%d" % i]).sum((1, 2)) / m["w%d" % i].sum((1, 2)).clamp_min(1.0)).sum()) for i in (1, 2)]
    eye = torch.eye(3, dtype=torch.float64)
    return ln[0] + ln[1] + mu * float(((torch.matmul(m["H1"], m["H2"]) - eye) ** 2).sum())


def main():
    install_standins()
    import importlib
    Rethinking = importlib.import_module("src.backbones.Rethinking")
    ResNet34 = importlib.import_module("src.backbones.ResNet34")
    PerceptualHead = importlib.import_module("src.heads.PerceptualHead")
    ransac_utils = importlib.import_module("src.heads.ransac_utils")
    for m in (Rethinking, ResNet34, PerceptualHead, ransac_utils):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(REF)), m.__file__
    from bihome_amd import configs
    torch.set_num_threads(8)
    import warnings
    warnings.filterwarnings("ignore")
    outdir = os.path.join(ROOT, "tests", "golden")
    Head, Aux = PerceptualHead.Model, PerceptualHead.AuxiliaryResnet

    def recorded(run):
        with Record(Aux, "forward") as feats, Record(Head, "_warp", static=True) as warps, \
                Record(ransac_utils.DSACSoftmax, "forward") as dsac, RecordFirstLinearInputs() as pre:
            r = run()
        return r, feats.calls, warps.calls, dsac.calls, pre.calls

    def state_dict_layout(cfg):
        sd = Aux(**cfg["MODEL"]["HEAD"]).state_dict()
        keys = [k for k in sd if k.startswith("projection_head.")]
        return dict(sd_keys=np.array(keys), sd_shapes=np.array([list(sd[k].shape) + [0] * (2 - sd[k].dim()) for k in keys]))

    def subsampled(pre, names, every=1):
        return {"pre_" + name: x[::every if name in ("f1", "f2") else 1, ::SUB, ::SUB] for name, x in zip(names, pre)}

    # ---- one-line: l1 with one hypothesis, cosine with four ---------------------------------------------------------------------
    for name, base, n in (("zeng_ihome_proj_b4", "zeng-ihome", 1), ("zeng_ihome_cos_proj_n4_b4", "zeng-ihome-cos", N_HYP)):
        cosine = base.endswith("cos")

        def config(margin):
            cfg = configs.get(base)
            cfg["MODEL"]["HEAD"].update(TRIPLET_MARGIN=margin, WITH_PROJECTION_HEAD=WIDTHS)
            if n > 1:
                cfg["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=n, POINTS_PER_HYPOTHESIS=N_PTS)
            return cfg

        def run(margin, dtype, steps):
            return recorded(lambda: run_bihome_variant(Rethinking.Model, Head, config(margin), dtype, batch=BATCH, seed=SEED, steps=steps))
        _, feats, warps, _, _ = run(1.0, torch.float64, 1)          # the step-0 maps do not depend on the margin
        probe = oneline_maps(feats, warps, cosine)
        margin = first_of_ladder(lambda m: oneline_share(probe, m))
        print(name, "shares over the ladder", [(round(m, 4), round(oneline_share(probe, m), 3)) for m in LADDER[:16:2]], "-> margin", margin)
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            r, feats, warps, dsac, pre = run(margin, dtype, 2)
            maps = oneline_maps(feats, warps, cosine)
            scores = dsac[0][1].reshape(-1) if n > 1 else None
            share = oneline_share(maps, margin)
            assert 0.2 <= share <= 0.8, share
            r.update(margin=np.float64(margin), active_share=np.float64(share), **state_dict_layout(config(margin)))
            if tag == "f64":
                assert maps["l1"].shape == (BATCH * n, 32, 32) and len(feats) == 6 and len(warps) == 4 and len(pre) == 6
                assert min(float(torch.norm(c[0], p=2, dim=1).min()) for c in feats[:3]) > 0           # no zero projected vector
                restated = oneline_loss(maps, margin, scores)
                assert abs(restated - r["loss"][0]) <= 1e-9 * abs(r["loss"][0]), (restated, r["loss"][0])
                r.update(maps)
                r.update(subsampled(pre[:3], ("f1", "f2", "f1w"), every=n))
                if scores is not None:
                    r["scores0"] = scores
            save(outdir, name, tag, r)

    # ---- double-line, string margin ----------------------------------------------------------------------------------------------
    def config():
        cfg = configs.get("detone-bihome")
        cfg["MODEL"]["HEAD"].update(WITH_PROJECTION_HEAD=WIDTHS)
        return cfg
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        r, feats, warps, _, pre = recorded(lambda: run_detone_steps(ResNet34.Model, Head, config(), dtype, batch=BATCH, seed=SEED, steps=2))
        r.update(margin=np.float64("inf"), active_share=np.float64(1.0), **state_dict_layout(config()))
        if tag == "f64":
            assert len(feats) == 8 and len(warps) == 8 and len(pre) == 8
            maps = bihome_maps(feats, warps)
            restated = bihome_loss(maps, config()["MODEL"]["HEAD"]["TRIPLET_MU"])
            assert abs(restated - r["loss"][0]) <= 1e-9 * abs(r["loss"][0]), (restated, r["loss"][0])
            r.update(maps)
            r.update(subsampled(pre[:4], ("f1", "f2", "f1w", "f2w")))
        save(outdir, "detone_bihome_proj_b4", tag, r)


if __name__ == "__main__":
    main()
