"""Write the fixtures of the two loss branches added after the shipped configs - the one-line loss on cosine distances
(PerceptualHead.py:485-499) and the double-line loss with a numeric margin and 'channel-aware' aggregation (:624-625, 644-645) - by
running the REFERENCE's own Rethinking.py, ResNet34.py and PerceptualHead.py through the stand-ins of oracle/make_golden.py.  Runs only
where the reference tree exists (never on the GPU box).

    python tools/make_golden_loss_variants.py

tests/golden/zeng_ihome_cos_b4_{f32,f64}.npz          zeng-ihome-cos, one hypothesis, two Adam steps on synth.make_pairs(4, seed=23)
tests/golden/zeng_ihome_cos_n4_b4_{f32,f64}.npz       the same with RANSAC_HYPOTHESIS_NO = 4, POINTS_PER_HYPOTHESIS = 16 (scores, rep = 4)
tests/golden/detone_bihome_aware_b4_{f32,f64}.npz     detone-bihome-aware, two Adam steps on the same batch
Each holds what oracle.make_golden.run_bihome_variant / run_detone_steps record, the chosen `margin`, the recorded `active_share`, and -
float64 files only - small per-pixel maps of step 0, computed HERE in float64 from the extractor outputs the reference produced
(recorded by wrapping AuxiliaryResnet.forward) and the warped all-ones masks (Model._warp):
  cosine          c13, c1w, w  [B*n,32,32] (and scores0 [B*n] for n = 4)
  channel-aware   M1, M2, w1, w2 [B,32,32] and the two homographies H1, H2 [B,3,3] of the mu term
The loss restated from these maps is asserted equal to the reference's step-0 loss to 1e-9 relative: that ties the formulas the kernels
implement (include/bihome.h) to upstream.

The margins are chosen HERE from a float64 run and stored (at the configs' margin of 1.0 the cosine hinge is active almost everywhere and
a fixture would not test it): the first value of the ladder 2^(-k/2), k = 0, 1, ... (rounded to float32) at which the share of active
hinge terms at step 0 lies in [0.2, 0.8] - cosine: over the pixels with w > 0; channel-aware: over all pixel-channel terms of both
directions.  Asserted again on what the two-step run records."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF, install_standins, run_bihome_variant, run_detone_steps  # noqa: E402

SEED, BATCH, N_HYP, N_PTS = 23, 4, 4, 16
EPS = 1e-8
LADDER = [float(np.float32(2.0 ** (-k / 2.0))) for k in range(60)]


class Record:
    """Wrap a function attribute of `owner` and keep (a float64 copy of) every tensor it returns, call by call."""

    def __init__(self, owner, name, static=False):
        self.owner, self.name, self.static, self.calls = owner, name, static, []

    def __enter__(self):
        self._orig = orig = self.owner.__dict__[self.name]
        fn = orig.__func__ if self.static else orig
        calls = self.calls

        def wrapped(*a, **k):
            out = fn(*a, **k)
            calls.append(tuple(x.detach().double().clone() for x in (out if isinstance(out, tuple) else (out,))))
            return out
        setattr(self.owner, self.name, staticmethod(wrapped) if self.static else wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self._orig)


def cos(x, y):
    """c(x, y) over dim 1: each norm clamped on its own (torch.cosine_similarity)."""
    nx, ny = x.pow(2).sum(1).sqrt().clamp_min(EPS), y.pow(2).sum(1).sqrt().clamp_min(EPS)
    return (x * y).sum(1) / (nx * ny)


def pooled(mask, size):
    return torch.nn.functional.avg_pool2d(mask, mask.shape[-1] // size)[:, 0]


def cosine_maps(feats, warps):
    f1, f2, f1w = (c[0] for c in feats[:3])
    w = pooled(warps[1][0], f1.shape[-1])                  # (patch_2's mask is all ones: its pooled map is 1)
    return dict(c13=cos(f1, f2), c1w=cos(f1w, f2), w=w)


def cosine_loss(m, margin, scores=None):
    t = (m["c13"] - m["c1w"] + margin).clamp_min(0)
    per = (m["w"] * t).sum((1, 2)) / m["w"].sum((1, 2)).clamp_min(1.0)
    return float((per * (1.0 if scores is None else scores)).sum())


def cosine_share(m, margin):
    on = m["w"] > 0
    return float(((m["c13"] - m["c1w"] + margin) > 0)[on].double().mean())


def aware_terms(feats, margin):
    f1, f2, f1w, f2w = (c[0] for c in feats[:4])
    l3 = (f1 - f2).abs()
    return (f1w - f2).abs() - l3 + margin, (f2w - f1).abs() - l3 + margin


def aware_maps(feats, warps, margin):
    t1, t2 = aware_terms(feats, margin)
    size = t1.shape[-1]
    return dict(M1=t1.clamp_min(0).sum(1), M2=t2.clamp_min(0).sum(1), w1=pooled(warps[1][0], size), w2=pooled(warps[3][0], size),
                H1=warps[0][1], H2=warps[2][1])


def aware_loss(m, mu):
    ln = [float(((m["w%d" % i] * m["M%d" % i]).sum((1, 2)) / m["w%d" % i].sum((1, 2)).clamp_min(1.0)).sum()) for i in (1, 2)]
    eye = torch.eye(3, dtype=torch.float64)
    return ln[0] + ln[1] + mu * float(((torch.matmul(m["H1"], m["H2"]) - eye) ** 2).sum())


def aware_share(feats, margin):
    t1, t2 = aware_terms(feats, margin)
    return float(torch.cat([(t1 > 0).reshape(-1), (t2 > 0).reshape(-1)]).double().mean())


def first_of_ladder(share):
    for margin in LADDER:
        if 0.2 <= share(margin) <= 0.8:
            return margin
    raise AssertionError("no margin of the ladder gives an active share in [0.2, 0.8]: %s" % [(m, share(m)) for m in LADDER[::6]])


def save(outdir, name, tag, r):
    path = os.path.join(outdir, "%s_%s.npz" % (name, tag))
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r.items()})
    size = os.path.getsize(path)
    print(path, size, "bytes; loss", r["loss"], "mace", r["mace"], "margin", r["margin"], "active share", r.get("active_share"))
    assert size < (1 << 20), (path, size)


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
                Record(ransac_utils.DSACSoftmax, "forward") as dsac:
            r = run()
        return r, feats.calls, warps.calls, dsac.calls

    # ---- one-line cosine: n = 1 and n = 4 ---------------------------------------------------------------------------------------
    for name, n in (("zeng_ihome_cos_b4", 1), ("zeng_ihome_cos_n4_b4", N_HYP)):
        def config(margin):
            cfg = configs.get("zeng-ihome-cos")
            cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = margin
            if n > 1:
                cfg["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=n, POINTS_PER_HYPOTHESIS=N_PTS)
            return cfg

        def run(margin, dtype, steps):
            return recorded(lambda: run_bihome_variant(Rethinking.Model, Head, config(margin), dtype, batch=BATCH, seed=SEED, steps=steps))
        _, feats, warps, _ = run(1.0, torch.float64, 1)          # the step-0 maps do not depend on the margin
        probe = cosine_maps(feats, warps)
        margin = first_of_ladder(lambda m: cosine_share(probe, m))
        print(name, "shares over the ladder", [(round(m, 4), round(cosine_share(probe, m), 3)) for m in LADDER[:16:2]], "-> margin", margin)
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            r, feats, warps, dsac = run(margin, dtype, 2)
            maps = cosine_maps(feats, warps)
            scores = dsac[0][1].reshape(-1) if n > 1 else None
            share = cosine_share(maps, margin)
            assert 0.2 <= share <= 0.8, share
            r.update(margin=np.float64(margin), active_share=np.float64(share))
            if tag == "f64":
                assert maps["c13"].shape == (BATCH * n, 32, 32) and len(feats) == 6 and len(warps) == 4
                restated = cosine_loss(maps, margin, scores)
                assert abs(restated - r["loss"][0]) <= 1e-9 * abs(r["loss"][0]), (restated, r["loss"][0])
                r.update(maps)
                if scores is not None:
                    r["scores0"] = scores
            save(outdir, name, tag, r)

    # ---- double-line, numeric margin, channel-aware -------------------------------------------------------------------------------
    def config(margin):
        cfg = configs.get("detone-bihome-aware")
        cfg["MODEL"]["HEAD"]["TRIPLET_MARGIN"] = margin
        return cfg

    def run(margin, dtype, steps):
        return recorded(lambda: run_detone_steps(ResNet34.Model, Head, config(margin), dtype, batch=BATCH, seed=SEED, steps=steps))
    _, feats, warps, _ = run(1.0, torch.float64, 1)
    margin = first_of_ladder(lambda m: aware_share(feats, m))
    print("detone_bihome_aware_b4 shares over the ladder", [(round(m, 4), round(aware_share(feats, m), 3)) for m in LADDER[:24:3]],
          "-> margin", margin)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        r, feats, warps, _ = run(margin, dtype, 2)
        share = aware_share(feats, margin)
        assert 0.2 <= share <= 0.8, share
        r.update(margin=np.float64(margin), active_share=np.float64(share))
        if tag == "f64":
            assert len(feats) == 8 and len(warps) == 8
            maps = aware_maps(feats, warps, margin)
            restated = aware_loss(maps, config(margin)["MODEL"]["HEAD"]["TRIPLET_MU"])
            assert abs(restated - r["loss"][0]) <= 1e-9 * abs(r["loss"][0]), (restated, r["loss"][0])
            r.update(maps)
        save(outdir, "detone_bihome_aware_b4", tag, r)


if __name__ == "__main__":
    main()
