"""The inference forward (`step.predict`: eval() under no_grad) of every backbone against the float64 oracle, with BatchNorm running
statistics that are not the initial (0, 1) (inference_cases.calibrated).

On this path net.run_forward defers each conv to its BatchNorm's position (plan.plan_folded), folds the running statistics into the
weights (net._folded) and fuses the ReLU / residual add into the conv epilogue (net._fw_folded_conv); the default 'f32' arithmetic
becomes the three-piece form.  What every BatchNorm position stores is captured by wrapping net._fw_folded_conv and the executor's
'bn' / 'tail' arms (net.py itself is untouched) and compared with the oracle's hooks.

Bound, everywhere: rel_l2(hip, float64 oracle) <= max(4 e32, 2^-20) with e32 = rel_l2(float32 oracle, float64 oracle) at the same tensor,
computed here (inference_cases.py says where the 4 and the 2^-20 come from).  No BatchNorm position may be skipped."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inference_cases as IC
from align_cases import textures
from bihome_amd import align, kernels as K, net
from oracle import bihome_oracle as O

pytestmark = pytest.mark.gpu

CONFIGS = ["zeng-bihome", "zeng-orig", "detone-bihome", "zhang-orig", "zhang-orig-trained-masks"]
BATCHES = {"b3": dict(batch=3), "b1": dict(batch=1), "b4": dict(batch=4), "b3-64x96": dict(batch=3, crop=(64, 96))}

_CAL, _REF = {}, {}


def calibration(name, seed=0, calib_seed=IC.CALIB_SEED, edit=None):
    """Module-wide cache of calibrated oracles; edit: name of a BatchNorm whose statistics go to the edges (IC.edit_statistics)."""
    key = (name, seed, calib_seed, edit)
    if key not in _CAL:
        if edit is None:
            _CAL[key] = IC.calibrated(name, seed, calib_seed)
        else:
            base = calibration(name, seed, calib_seed)
            _CAL[key] = base.with_state(IC.edit_statistics(base.sd, edit))
    return _CAL[key]


def fixed_choice(B, h, w):
    return O.sample_choice(h * w, B * 128, torch.Generator().manual_seed(3)).reshape(B, 128)


def reference(name, batch="b3", **cal_kw):
    """(calibration, numpy batch, choice, float64 run, float32 run): computed once per (config, weights, batch)."""
    key = (name, batch) + tuple(sorted(cal_kw.items()))
    if key not in _REF:
        cal = calibration(name, **cal_kw)
        b = IC.pairs(**BATCHES[batch])
        B, _, h, w = b["patch_1"].shape
        choice = fixed_choice(B, h, w)
        _REF[key] = (cal, b, choice) + IC.reference(cal, name, b, choice)
    return _REF[key]


def hip_model(name, precision, sd):
    from bihome_amd.step import build_model
    cfg = IC.config(name)
    cfg["MODEL"]["BACKBONE"]["PRECISION"] = precision
    model = build_model(cfg)
    model[0].load_state_dict(sd)
    return model.eval()


def set_fold(model, fold):
    runners = net.trainable_runners(model)          # the backbone's, and for ContentAware the extractor's and a trained mask predictor's
    for r in runners:
        r.fold_bn = fold
    return runners


def device_batch(b, choice):
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    B, P = b["patch_1"].shape[0], b["patch_1"].shape[-1]
    data["choice"] = choice.cuda()
    data["corners"] = torch.tensor([[0, 0], [P, 0], [P, P], [0, P]], dtype=torch.float32, device="cuda").repeat(B, 1, 1)
    return data


class Capture:
    """Records (op, what the op stored, stored as NCHW?) at every BatchNorm position of every conv stack that runs while it is installed,
    and in `split` the folded convs that ran on packed split-operand weights (the condition of net._fw_folded_conv, restated)."""

    def __init__(self, monkeypatch):
        self.records, self.folded, self.split = [], 0, []
        fold, bn, tail = net._fw_folded_conv, net._FW_ARMS["bn"], net._FW_ARMS["tail"]

        def fw_folded_conv(s, i, op):
            out = fold(s, i, op)
            self.folded += 1
            self.records.append((op, out, False))
            cop = s.prog.ops[s.plan.folded[i]]
            d = net._conv_geometry(cop.mod, s.slots[cop.src].shape, cop.extra["in_nchw"], cop.extra["out_nchw"], s.precision)
            if s.precision in K.SPLIT_PIECES and d.bh_packs and cop.extra["weight_fn"] is None:
                self.split.append((cop.mod, op))
            return out

        def fw_bn(s, i, op, src):
            out = bn(s, i, op, src)
            j = s.prog.index().producer.get(op.src)
            nchw = j is not None and s.prog.ops[j].kind == "conv" and bool(s.prog.ops[j].extra["out_nchw"])
            self.records.append((op, out, nchw))
            return out

        def fw_tail(s, i, op, src):
            out = tail(s, i, op, src)
            self.records.append((op, out, True))
            return out
        monkeypatch.setattr(net, "_fw_folded_conv", fw_folded_conv)
        monkeypatch.setitem(net._FW_ARMS, "bn", fw_bn)
        monkeypatch.setitem(net._FW_ARMS, "tail", fw_tail)


def check_taps(records, model, r64, r32, what, only=None):
    """The shared checker: every recorded BatchNorm position against the float64 oracle, bound max(4 e32, 2^-20); every BatchNorm the
    oracle ran must have been recorded (only: restrict both to these BatchNorm names).  Returns (worst err / e32, its name)."""
    names = {m: n for n, m in model[0].named_modules()}
    ran = {n for n, m in model[0].named_modules() if isinstance(m, torch.nn.BatchNorm2d) and n in r64.tap}
    seen, bad, worst = set(), [], (0.0, None)
    for op, out, nchw in records:
        name = names[op.mod[1]] if op.kind == "tail" else names[op.mod]
        if only is not None and name not in only:
            continue
        want64, want32 = IC.expected_at(op, r64.tap, names), IC.expected_at(op, r32.tap, names)
        if isinstance(out, K.BnPooled):             # BatchNorm + ReLU + MaxPool2d(3, 2, 1) in one pass: only the pooled map exists
            out, want64, want32 = out.pooled, F.max_pool2d(want64, 3, 2, 1), F.max_pool2d(want32, 3, 2, 1)
        assert torch.is_tensor(out), (name, type(out))
        got = out if nchw else out.permute(0, 3, 1, 2)
        err, e32 = IC.rel_l2(got, want64), IC.rel_l2(want32, want64)
        seen.add(name)
        if err / max(e32, 1e-30) > worst[0]:
            worst = (err / max(e32, 1e-30), name)
        if not err <= IC.bound(e32):
            bad.append((name, err, e32))
    missing = (ran if only is None else set(only)) - seen
    print("INFERENCE-PARITY %s: %d BatchNorm positions, worst err / e32 = %.2f at %s; %d past max(4 e32, 2^-20): %s"
          % (what, len(seen), worst[0], worst[1], len(bad), ["%s %.2e (e32 %.2e)" % b for b in bad[:6]]))
    assert not missing, ("BatchNorm positions without a recorded value", sorted(missing))
    assert not bad, bad[:10]
    return worst


def check_outputs(data, delta, r64, r32, what):
    """The backbone's outputs and delta_hat against the float64 oracle under the same bound."""
    bad = []
    for k in r64.out:
        err, e32 = IC.rel_l2(data[k], r64.out[k]), IC.rel_l2(r32.out[k], r64.out[k])
        print("INFERENCE-PARITY %s: %s err %.2e, e32 %.2e, err / e32 = %.2f" % (what, k, err, e32, err / e32))
        if not err <= IC.bound(e32):
            bad.append((k, err, e32))
    err, e32 = IC.rel_l2(delta.reshape(-1, 4, 2), r64.delta), IC.rel_l2(r32.delta, r64.delta)
    print("INFERENCE-PARITY %s: delta_hat err %.2e, e32 %.2e, err / e32 = %.2f" % (what, err, e32, err / max(e32, 1e-30)))
    if not err <= IC.bound(e32):
        bad.append(("delta_hat", err, e32))
    assert not bad, bad


def run_case(monkeypatch, name, fold, precision, batch="b3", edit=None):
    from bihome_amd.step import predict
    cal, b, choice, r64, r32 = reference(name, batch, **({"edit": edit} if edit else {}))
    model = hip_model(name, precision, cal.sd)
    runners = set_fold(model, fold)
    cap = Capture(monkeypatch)
    data = device_batch(b, choice)
    delta = predict(model, data)
    what = "%s %s fold=%s %s%s" % (name, batch, fold, precision, " edges at " + edit if edit else "")
    check_taps(cap.records, model, r64, r32, what)
    check_outputs(data, delta, r64, r32, what)
    planned = sum(len(r.prog.last_forward_plan.folded) for r in runners)
    print("INFERENCE-PARITY %s: %d folded convs, %d of them on packed split-operand weights" % (what, cap.folded, len(cap.split)))
    assert cap.folded == planned and len(cap.records) >= IC.BN_COUNT[name]
    if fold:
        assert planned > (50 if name.startswith("zeng") else 30)
    else:
        assert planned == 0
    return model, data, delta, cap


# ------------------------------------------------------------------------------------------------
# every backbone, folded and unfolded, in the three full-precision arithmetics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x3", "f32-mfma"])
@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("name", CONFIGS)
def test_backbone_inference_vs_oracle(monkeypatch, name, fold, precision):
    run_case(monkeypatch, name, fold, precision)


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("name,batch", [("zeng-orig", "b1"), ("zeng-bihome", "b1"), ("detone-bihome", "b1"), ("zeng-bihome", "b3-64x96")],
                         ids=["zeng-orig-N1", "zeng-bihome-N2", "detone-bihome-N2", "zeng-bihome-64x96"])
def test_batch_of_one_and_a_rectangular_map(monkeypatch, name, batch, fold):
    run_case(monkeypatch, name, fold, "f32", batch=batch)


EDGES = [("zeng-bihome", "layer3.1.upper_branch.1"),          # behind a 3x3 conv, mid-network
         ("zeng-bihome", "layer4.6.lower_branch.1"),          # behind the bias-free ConvTranspose2d of a deconv unit
         ("detone-bihome", "resnet34.layer2.1.bn1")]


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("name,bn", EDGES, ids=["zeng-3x3", "zeng-convT", "detone-3x3"])
def test_statistics_at_the_edges(monkeypatch, name, bn, fold):
    """running_var 0 and 1e6, running_mean +-1e3 and gamma 0 in one BatchNorm: the folded weights' dynamic range is unlike anything
    training produces.  The float32 oracle defines e32 on the same edited weights."""
    cal = calibration(name, edit=bn)
    mod = dict(cal.bb64.named_modules())[bn]
    assert mod.running_var[0] == 0 and mod.running_var[2] == 1e6 and mod.running_mean[5] == -1e3 and mod.weight[6] == 0
    model = run_case(monkeypatch, name, fold, "f32", edit=bn)[0]
    hip = dict(model[0].named_modules())[bn]
    assert hip.running_var[1].item() == 0 and hip.running_mean[4].item() == 1e3 and hip.weight[6].item() == 0


# ------------------------------------------------------------------------------------------------
# reduced-precision modes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x3"])
def test_split_operand_fold_on_several_layers(monkeypatch, precision):
    """Below 256 workgroups the halo-tiled 3x3 kernel leaves a conv to the generic kernel (csrc/conv3x3.hip C3_MIN_BLOCKS), so at the
    batch of 3 only the 128 x 128 layer runs on the packed split-operand copy of its folded weights.  At B = 4 (N = 8) the 64 x 64
    layers do too - among them a conv that closes a residual unit, whose add and ReLU ride in the packed kernel's epilogue."""
    cap = run_case(monkeypatch, "zeng-bihome", True, precision, batch="b4")[3]
    assert len(cap.split) >= 4 and any(op.res is not None for _, op in cap.split), len(cap.split)


@pytest.mark.parametrize("precision,bits", [("bf16", 8), ("f32x2", 16)])
@pytest.mark.parametrize("name", ["zeng-bihome", "detone-bihome"])
def test_reduced_modes_track_the_rounded_operand_oracle(monkeypatch, name, precision, bits):
    """'bf16' (bf16 MFMA operands) and 'f32x2' (two bf16 pieces per operand), folded: the error against float64 is at most 4 times that
    of the oracle run with the conv operands rounded to 8 / 16 significant bits, and at least 1/64 of it (the mode really ran).

    The emulation is corrected from the kernel source in two ways.  It rounds only the operands the kernels round: in 'bf16' every conv
    with a multiple of 32 input channels except the fp32 stem and fused tail (inference_cases.bf16_operand_convs); in 'f32x2' only the
    convs that run on packed two-piece weights - the halo-tiled 3x3 kernel, which below 256 workgroups leaves the launch to the generic
    fp32 kernel (csrc/conv3x3.hip C3_MIN_BLOCKS): at this batch one layer of the Zeng backbone and none of the DeTone regressor, read
    off the run itself.  And it runs on the float32 oracle, because everything else in the kernels - accumulation, storage, the layers
    that are not rounded - is fp32: where no layer is rounded the 'f32x2' reference is the float32 oracle itself and the upper bound is
    the one of the full-precision tests."""
    from bihome_amd.step import predict
    cal, b, choice, r64, _ = reference(name)
    model = hip_model(name, precision, cal.sd)
    cap = Capture(monkeypatch)
    data = device_batch(b, choice)
    delta = predict(model, data)
    assert cap.folded > 30
    names = {m: n for n, m in model[0].named_modules()}
    split = sorted(names[m] for m, _ in cap.split)
    if precision == "f32x2":
        only = frozenset(split)
        assert len(only) == (1 if name == "zeng-bihome" else 0), split
    else:
        only = frozenset(IC.bf16_operand_convs(cal.bb32, name))
        assert not split and len(only) >= 35
    print("INFERENCE-PARITY %s %s: %d convs with rounded operands%s" % (name, precision, len(only), (": " + ", ".join(split)) if split else ""))
    key = (name, "rounded", bits, only)
    if key not in _REF:
        _REF[key] = IC.oracle_run(cal, name, b, choice, torch.float32, rounded=(bits, only))
    rr = _REF[key]
    bad = []
    for what, got, want, emu in [(k, data[k], r64.out[k], rr.out[k]) for k in r64.out] + [("delta_hat", delta.reshape(-1, 4, 2), r64.delta, rr.delta)]:
        err, model_err = IC.rel_l2(got, want), IC.rel_l2(emu, want)
        print("INFERENCE-PARITY %s %s: %s err %.2e, rounded-operand oracle %.2e, ratio %.2f" % (name, precision, what, err, model_err, err / model_err))
        if not model_err / 64 <= err <= 4 * model_err:
            bad.append((what, err, model_err))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# folded weights follow the parameters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeng-bihome", "detone-bihome"])
def test_reload_refolds(monkeypatch, name):
    """After a folded predict a second calibrated state dict goes into the same model: the next predict is the second weights' (bound
    against their oracle) and far from the first (a stale fold would repeat it)."""
    from bihome_amd.step import predict
    model, data1, delta1, _ = run_case(monkeypatch, name, True, "f32")
    first = {k: data1[k].clone() for k in IC.output_keys(calibration(name).cfg) if k in data1}
    cal2, b, choice, r64, r32 = reference(name, seed=3, calib_seed=32)
    model[0].load_state_dict(cal2.sd)
    cap = Capture(monkeypatch)
    data2 = device_batch(b, choice)
    delta2 = predict(model, data2)
    check_taps(cap.records, model, r64, r32, "%s reloaded" % name)
    check_outputs(data2, delta2, r64, r32, "%s reloaded" % name)
    for k in first:
        moved, limit = IC.rel_l2(data2[k], first[k]), 100 * IC.bound(IC.rel_l2(r32.out[k], r64.out[k]))
        assert moved > limit, (k, moved, limit)


TEETH = [("zeng-bihome", "layer3.1.upper_branch.1"), ("detone-bihome", "resnet34.layer2.1.bn1")]


@pytest.mark.parametrize("name,bn", TEETH, ids=["zeng", "detone"])
def test_the_bound_has_teeth(monkeypatch, name, bn):
    """One folded weight tensor scaled by 1 + 2^-11 on the host (4.9e-4: below both bounds of the fold-against-unfold test, above 4 times
    the largest e32): the tap check at that layer fails, the layers in front of it still pass."""
    from bihome_amd.step import predict
    cal, b, choice, r64, r32 = reference(name)
    model = hip_model(name, "f32", cal.sd)
    target = dict(model[0].named_modules())[bn]
    folded, hits = net._folded, []

    def bent(cache, conv, bnm, weight_fn):
        wf, bf = folded(cache, conv, bnm, weight_fn)
        if bnm is target:
            hits.append(1)
            wf = wf * (1.0 + 2.0 ** -11)
        return wf, bf
    monkeypatch.setattr(net, "_folded", bent)
    cap = Capture(monkeypatch)
    predict(model, device_batch(b, choice))
    assert hits
    order = [n for n, m in model[0].named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    before = set(order[:order.index(bn)])
    check_taps(cap.records, model, r64, r32, "%s bent, in front of %s" % (name, bn), only=before)
    with pytest.raises(AssertionError):
        check_taps(cap.records, model, r64, r32, "%s bent at %s" % (name, bn), only={bn})


# ------------------------------------------------------------------------------------------------
# the Aligner with a real model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeng-bihome", "detone-orig"])
def test_aligner_with_a_calibrated_model(monkeypatch, name):
    """delta_hat and H of Aligner(model) on two texture pairs against the oracle run on the patches the aligner made, with the same
    point draws and corners.  H: against align.lift of the float64 oracle's delta, within what the delta bound implies through lift -
    measured by lifting the float32 oracle's delta."""
    cal = calibration(name)
    model = hip_model(name, "f32", cal.sd)
    choice = fixed_choice(2, 128, 128)
    if hasattr(model[1], "sample_choice"):
        monkeypatch.setattr(model[1], "sample_choice", lambda n_points, count, device: choice.reshape(-1)[:count].to(device), raising=False)
    aligner = align.Aligner(model, patch=128)
    a = torch.from_numpy(textures(2, 240, 320, seed=1)).cuda()
    b = torch.from_numpy(textures(2, 120, 200, seed=2)).cuda()
    r = aligner(a, b, warp=False)
    batch = {"patch_1": r["patch_1"].cpu().numpy(), "patch_2": r["patch_2"].cpu().numpy()}
    r64, r32 = IC.reference(cal, name, batch, choice)
    err, e32 = IC.rel_l2(r["delta_hat"], r64.delta), IC.rel_l2(r32.delta, r64.delta)
    print("INFERENCE-PARITY aligner %s: delta_hat err %.2e, e32 %.2e, err / e32 = %.2f" % (name, err, e32, err / e32))
    assert r["delta_hat"].shape == (2, 4, 2) and err <= IC.bound(e32)
    ga, gb = r["geom_a"].cpu().numpy(), r["geom_b"].cpu().numpy()
    H64, H32 = align.lift(r64.delta.numpy(), 128, ga, gb), align.lift(r32.delta.double().numpy(), 128, ga, gb)
    H = r["H"].cpu().numpy()
    for s in range(2):
        eh, eh32 = IC.rel_l2(H[s], H64[s]), IC.rel_l2(H32[s], H64[s])
        print("INFERENCE-PARITY aligner %s: H[%d] err %.2e, float32 oracle's delta lifted %.2e" % (name, s, eh, eh32))
        assert eh <= IC.bound(eh32), (s, eh, eh32)
