"""Write the fixtures of the DSAC inlier-count scorers ('inliers_ratio' / 'soft_inliers_ratio', ransac_utils.py:98-111) by running the
REFERENCE's own Rethinking.py, PerceptualHead.py and ransac_utils.py through the stand-ins of oracle/make_golden.py.  Runs only where
the reference tree exists (never on the GPU box).

    python tools/make_golden_dsac_scoring.py

tests/golden/{zeng_ihome,zeng_multihead}_soft_n4_b4_{f32,f64}.npz: the base config with RANSAC_HYPOTHESIS_NO = 4,
POINTS_PER_HYPOTHESIS = 16, SCORING_METHOD = 'soft_inliers_ratio' on synth.make_pairs(4, seed=19), two Adam steps - everything
oracle.make_golden.run_bihome_variant records for the *_n4_b4 fixtures, plus the step-0 hypotheses `H0` [4,4,3,3] and their softmax
weights `scores0` [4,4], and an eval-mode predict_homography at the initial weights for both methods (`eval_choice`, `eval_H`,
`eval_best_{soft,hard}`, `eval_delta_hat_{soft,hard}`, `eval_raw_{soft,hard}`).  tests/golden/zeng_soft_n4_b4_{map0,mapeval}_f64.npz: the
float64 map fields (coordinates + perspective field, [4, 16384, 2]) of step 0 and of the eval run - the same for both configs (one
backbone), asserted here - from which tests/test_dsac_scoring_cpu.py restates the scores.

The parameters are chosen HERE, from the float64 run, so that the scores test something (at a random-initialised field a small
threshold saturates every sigmoid and the softmax comes out uniform; a large beta makes it one-hot), and stored in the fixtures:
  thr       the median step-0 point distance over the batch (all hypotheses), rounded to float32;
  beta      the first value of 10 * 2^(-k/2), k = 0, 1, ... (rounded to float32) at which all 4 samples - failing that, 3 of the 4 -
            have a largest step-0 weight in [0.3, 0.97]; at least 3 of 4 is asserted again on the weights the run then records;
  eval_thr_soft, eval_beta   the same rule on the distances of the eval run (at the initial running statistics the field is of another
            magnitude than in training mode), with one more condition because this run PICKS: the two lowest raw scores of every sample
            are at least 0.2 apart, and - asserted after both runs - at least 10 times as far apart as the reference's own float32 and
            float64 runs disagree on the raw-score differences;
  eval_thr_hard   the hard method's threshold for the eval run: the centre of the gap of the sorted eval distances nearest their median
            that keeps every distance more than 1e-3 away and makes every sample's minimal count unique, so that an fp32 device picks
            the same hypothesis as the float64 run.  Both conditions are asserted."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF, RecordMultinomial, install_standins, run_bihome_variant, t  # noqa: E402

SEED, BATCH, N_HYP, N_PTS = 19, 4, 4, 16
CLEAR = 1e-3


class RecordDsac:
    """Wrap DSACSoftmax.forward to record its inputs and outputs: (points1, points2, homographies, scores) per call."""

    def __init__(self, cls):
        self.cls, self.calls = cls, []

    def __enter__(self):
        self._orig = orig = self.cls.forward
        calls = self.calls

        def forward(mod, points1, points2, *a, **k):
            H, s = orig(mod, points1, points2, *a, **k)
            calls.append(tuple(x.detach().double().clone() for x in (points1, points2, H, s)))
            return H, s
        self.cls.forward = forward
        return self

    def __exit__(self, *exc):
        self.cls.forward = self._orig


def distances(H, p1, p2):
    """Point distances of every hypothesis, float64: H [B,n,3,3], p1 / p2 [B,N,2] -> e [B,n,N]."""
    ph = torch.cat([p1, torch.ones_like(p1[..., :1])], -1)
    q = torch.einsum("bnij,bpj->bnpi", H, ph)
    z = q[..., 2:]
    big = z.abs() > 1e-8
    scale = torch.where(big, 1.0 / torch.where(big, z, torch.ones_like(z)), torch.ones_like(z))
    return (q[..., :2] * scale - p2[:, None]).norm(dim=-1)


def soft_weights(e, thr, beta):
    return torch.softmax(-torch.sigmoid(beta * (e - thr)).sum(-1), -1)


def informative(w):
    top = w.max(-1).values
    return int(((top >= 0.3) & (top <= 0.97)).sum()) >= 3


def f32(v):
    return float(np.float32(v))


def pick_gap(w):
    """log(largest weight / second largest) per sample = the distance between the two lowest raw scores."""
    top = torch.sort(w, -1, descending=True).values
    return torch.log(top[:, 0] / top[:, 1])


def choose_soft(e, min_gap=0.0):
    """thr = the median distance; beta = the first 10 * 2^(-k/2) with all samples (failing that: 3 of 4) informative and, for a run
    that picks a hypothesis, the two best raw scores of every sample at least min_gap apart."""
    thr = f32(e.median())
    for need in (e.shape[0], 3):
        for k in range(120):
            beta = f32(10.0 * 2.0 ** (-k / 2.0))
            w = soft_weights(e, thr, beta)
            top = w.max(-1).values
            if int(((top >= 0.3) & (top <= 0.97)).sum()) >= need and float(pick_gap(w).min()) >= min_gap:
                return thr, beta
    raise AssertionError("no beta makes the weights informative")


def choose_hard(e):
    """-> thr (float32-representable) in a gap of the distances: nothing within CLEAR, every sample's minimal count unique."""
    v = np.sort(e.numpy().ravel())
    lo = np.nonzero(v[1:] - v[:-1] > 2.5 * CLEAR)[0]
    mids = (v[lo] + v[lo + 1]) / 2
    med = np.median(v)
    for thr in mids[np.argsort(np.abs(mids - med))]:
        thr = f32(thr)
        if hard_conditions(e, thr):
            return thr
    raise AssertionError("no threshold gives a well-defined hard pick")


def hard_conditions(e, thr):
    if float((e - thr).abs().min()) <= CLEAR:
        return False
    cnt = (e < thr).sum(-1)
    return all(int((cnt[b] == cnt[b].min()).sum()) == 1 for b in range(cnt.shape[0]))


def run_eval(bb_cls, head_cls, dsac_cls, cfg, dtype, soft, thr_hard):
    """Eval-mode predict_homography at the initial weights with both methods on the same draws.  soft = (thr, beta) and thr_hard:
    None in the float64 run, which chooses them."""
    from bihome_amd import synth
    from bihome_amd.weights import load_synthetic
    bb = bb_cls(**cfg["MODEL"]["BACKBONE"])
    head = head_cls(bb, **cfg["MODEL"]["HEAD"])
    load_synthetic(bb, seed=0)
    load_synthetic(head.auxiliary_resnet, seed=0)
    model = torch.nn.Sequential(bb, head).to(dtype).eval()
    d = synth.make_pairs(BATCH, seed=SEED)
    out = {}
    with torch.no_grad():
        data = bb.predict_homography({k: t(d[k], dtype) for k in ("patch_1", "patch_2", "delta")})
        if soft is None:            # a first pass for the distances alone: the hypotheses do not depend on the parameters
            torch.manual_seed(2000)
            with RecordDsac(dsac_cls) as dsac:
                head.predict_homography(dict(data))
            e = distances(dsac.calls[0][2], dsac.calls[0][0], dsac.calls[0][1])
            soft, thr_hard = choose_soft(e, min_gap=0.2), choose_hard(e)
        thr, beta = soft
        for method in ("soft", "hard"):
            head.dsac.scoring_method = {"soft": "soft_inliers_ratio", "hard": "inliers_ratio"}[method]
            head.dsac.scoring_distance_threshold = thr if method == "soft" else thr_hard
            head.dsac.scoring_distance_beta = beta
            torch.manual_seed(2000)
            with RecordMultinomial() as rec, RecordDsac(dsac_cls) as dsac:
                dh, _ = head.predict_homography(dict(data))
            p1, p2, H, w = dsac.calls[0]
            if method == "soft":
                out.update(eval_choice=rec.calls[0].reshape(BATCH, -1).numpy(), eval_H=H.numpy().copy(), eval_map=p2.numpy().copy())
                e = distances(H, p1, p2)
                out.update(eval_thr_hard=np.float64(thr_hard), eval_thr_soft=np.float64(thr), eval_beta=np.float64(beta),
                           eval_scores_soft=w.numpy().copy())
                out["eval_raw_soft"] = torch.sigmoid(beta * (e - thr)).sum(-1).numpy()
                out["eval_raw_hard"] = ((e < thr_hard).sum(-1).double() / e.shape[-1]).numpy()
                out["eval_e"] = e
            else:
                assert np.array_equal(rec.calls[0].reshape(BATCH, -1).numpy(), out["eval_choice"]) and np.array_equal(H.numpy(), out["eval_H"])
            out["eval_best_" + method] = torch.argmax(w, -1).numpy()
            out["eval_delta_hat_" + method] = dh.double().numpy().copy()
    return out


def main():
    install_standins()
    import importlib
    Rethinking = importlib.import_module("src.backbones.Rethinking")
    PerceptualHead = importlib.import_module("src.heads.PerceptualHead")
    ransac_utils = importlib.import_module("src.heads.ransac_utils")
    for m in (Rethinking, PerceptualHead, ransac_utils):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(REF)), m.__file__
    from bihome_amd import configs
    torch.set_num_threads(8)
    import warnings
    warnings.filterwarnings("ignore")
    outdir = os.path.join(ROOT, "tests", "golden")

    def config(base, thr, beta):
        cfg = configs.get(base)
        cfg["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=N_HYP, POINTS_PER_HYPOTHESIS=N_PTS, SCORING_METHOD="soft_inliers_ratio",
                                    SCORING_DISTANCE_THRESHOLD=thr, SCORING_DISTANCE_BETA=beta)
        return cfg

    # the parameters: one float64 step of zeng-ihome with placeholders - the hypotheses and the distances do not depend on them
    with RecordDsac(ransac_utils.DSACSoftmax) as dsac:
        run_bihome_variant(Rethinking.Model, PerceptualHead.Model, config("zeng-ihome", 1.0, 1.0), torch.float64, batch=BATCH, seed=SEED,
                           steps=1)
    p1, p2, H, _ = dsac.calls[0]
    e0 = distances(H, p1, p2)
    thr, beta = choose_soft(e0)
    print("step-0 distances: median %.4f, quartiles %.3f / %.3f -> thr %.6f beta %.6g" % (e0.median(), e0.quantile(0.25), e0.quantile(0.75), thr, beta))
    print("step-0 weights at the choice\n", soft_weights(e0, thr, beta).numpy())

    ev_soft, thr_hard, maps = None, None, {}
    for base, loss_name in (("zeng-ihome", None), ("zeng-multihead", "L1Loss")):
        name = base.replace("-", "_") + "_soft_n4_b4"
        picks = {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            cfg = config(base, thr, beta)
            with RecordDsac(ransac_utils.DSACSoftmax) as dsac:
                r = run_bihome_variant(Rethinking.Model, PerceptualHead.Model, cfg, dtype, batch=BATCH, seed=SEED, steps=2, loss_name=loss_name)
            q1, q2, H0, w0 = dsac.calls[0]
            r.update(H0=H0.numpy(), scores0=w0.numpy(), thr=np.float64(thr), beta=np.float64(beta))
            ev = run_eval(Rethinking.Model, PerceptualHead.Model, ransac_utils.DSACSoftmax, cfg, dtype, ev_soft, thr_hard)
            e_eval, map_eval = ev.pop("eval_e"), ev.pop("eval_map")
            if tag == "f64":
                assert informative(w0), w0
                assert (soft_weights(distances(H0, q1, q2), thr, beta) - w0).abs().max() < 1e-9
                ev_soft, thr_hard = (float(ev["eval_thr_soft"]), float(ev["eval_beta"])), float(ev["eval_thr_hard"])
                assert hard_conditions(e_eval, thr_hard)
                assert informative(torch.from_numpy(ev["eval_scores_soft"])) and float(pick_gap(torch.from_numpy(ev["eval_scores_soft"])).min()) >= 0.2
                for key, val in (("map0", q2.numpy()), ("mapeval", map_eval)):
                    assert key not in maps or np.array_equal(maps[key], val), "the two configs do not share their fields"
                    maps[key] = val
                print(name, "eval thr_hard %.6f nearest distance %.2e counts\n" % (thr_hard, float((e_eval - thr_hard).abs().min())),
                      (e_eval < thr_hard).sum(-1).numpy(), "\nsoft raw\n", ev["eval_raw_soft"])
            picks[tag] = (ev["eval_best_soft"], ev["eval_best_hard"], ev["eval_scores_soft"])
            r.update(ev)
            np.savez_compressed(os.path.join(outdir, "%s_%s.npz" % (name, tag)), **r)
            print(name, tag, "loss", r["loss"], "mace", r["mace"], "scores0\n", r["scores0"], "\neval picks", picks[tag][:2])
        for a, b in zip(picks["f32"][:2], picks["f64"][:2]):
            assert np.array_equal(a, b), ("the reference's own float32 and float64 runs pick differently", picks)
        w32, w64 = (torch.from_numpy(picks[k][2]).double().clamp_min(1e-300) for k in ("f32", "f64"))
        d32, d64 = (-(torch.log(w) - torch.log(w.max(-1, keepdim=True).values)) for w in (w32, w64))      # raw score minus the lowest one
        spread = float((d32 - d64)[w64 > 1e-30].abs().max())
        print(name, "eval soft: gap between the two lowest raw scores", pick_gap(w64).numpy(), "float32 / float64 spread %.3e" % spread)
        assert float(pick_gap(w64).min()) >= 10 * spread
    for key, val in maps.items():
        path = os.path.join(outdir, "zeng_soft_n4_b4_%s_f64.npz" % key)
        np.savez_compressed(path, map=val)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
