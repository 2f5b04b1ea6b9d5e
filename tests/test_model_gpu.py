"""End-to-end parity of the drop-in modules (HIP path) with the CPU oracle and with the golden vectors
captured from the reference's own files.  Sizes are the reference's CPU-runnable case (B=8) or smaller."""
import numpy as np
import pytest
import torch

from bihome_amd import configs, synth
from bihome_amd.weights import load_synthetic
from oracle import bihome_oracle as O

pytestmark = pytest.mark.gpu


def cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda()


def relerr(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref).max() / (np.abs(ref).max() + 1e-30)


@pytest.fixture(scope="module")
def zeng():
    from bihome_amd.step import build_model
    cfg = configs.get("zeng-bihome")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    return cfg, model


def test_plugin_discovery_and_state_dict_keys(zeng):
    import importlib
    cfg, model = zeng
    assert importlib.import_module("src.backbones.Rethinking").Model is type(model[0])
    assert importlib.import_module("src.heads.PerceptualHead").Model is type(model[1])
    bb, head = O.build(cfg)
    assert set(torch.nn.Sequential(bb, head).state_dict().keys()) == set(model.state_dict().keys())


def test_no_cpu_fallback(zeng):
    cfg, model = zeng
    d = synth.make_pairs(2, seed=1)
    with pytest.raises(RuntimeError, match="no CPU"):
        model[0]({k: torch.tensor(d[k]) for k in ("patch_1", "patch_2")})


def backbone_reference(cfg, d):
    """The oracle backbone on the patch pairs d["patch_1"], d["patch_2"] [B,1,h,w] in float32 and float64, with the output gradients g12, g21:
    {dtype: (outputs, parameter gradients, module)}, g12, g21, and the float32 run's whole-gradient relative L2 distance from the float64 run."""
    B, _, h, w = d["patch_1"].shape
    rng = np.random.Generator(np.random.PCG64(0))
    g12, g21 = rng.standard_normal((B, 2, h, w)), rng.standard_normal((B, 2, h, w))
    ref = {}
    for dt in (torch.float32, torch.float64):
        bb, _ = O.build(cfg)
        load_synthetic(bb, 0)
        bb.to(dt).train()
        o = bb({k: torch.tensor(d[k], dtype=dt) for k in ("patch_1", "patch_2")})
        ((o["pf_hat_12"] * torch.tensor(g12, dtype=dt)).sum() + (o["pf_hat_21"] * torch.tensor(g21, dtype=dt)).sum()).backward()
        ref[dt] = ({k: o[k].detach().double() for k in ("pf_hat_12", "pf_hat_21")},
                   {n: p.grad.double() for n, p in bb.named_parameters()}, bb)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    spread = (sum((g32[n] - g64[n]).pow(2).sum().item() for n in g64) / sum(g64[n].pow(2).sum().item() for n in g64)) ** 0.5
    return ref, g12, g21, spread


def check_backbone_forward_backward_vs_oracle(zeng, d, reference=None):
    """Backbone alone on the patch pairs d["patch_1"], d["patch_2"] [B,1,h,w]: outputs against the float64 oracle; parameter gradients
    against the float64 oracle with a tolerance tied to the oracle's own float32-vs-float64 spread (at a tiny batch a few
    ReLU sign flips move some gradients by several percent even between two CPU precisions).  reference: backbone_reference(cfg, d), if
    the caller has it already."""
    cfg, model = zeng
    B, _, h, w = d["patch_1"].shape
    ref, g12, g21, _ = reference if reference is not None else backbone_reference(cfg, d)
    out64, grad64, bb64 = ref[torch.float64]
    out32, grad32, _ = ref[torch.float32]
    model.train()
    load_synthetic(model[0], 0)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2")}
    out = model[0](data)
    for k in ("pf_hat_12", "pf_hat_21"):
        assert out[k].shape == (B, 2, h, w) and out[k].is_contiguous()
        print("MEASURED backbone %dx%d %s: error %.3e of max |pf| (float32 oracle's own %.3e)" % (h, w, k, relerr(out[k].detach().cpu(), out64[k]), relerr(out32[k], out64[k])))
        assert relerr(out[k].detach().cpu(), out64[k]) < max(3 * relerr(out32[k], out64[k]), 1e-5), k
    for p in model[0].parameters():
        p.grad = None
    ((out["pf_hat_12"] * cuda(g12)).sum() + (out["pf_hat_21"] * cuda(g21)).sum()).backward()
    gscale = max(g.abs().max().item() for g in grad64.values())
    bad, num, den, num32 = [], 0.0, 0.0, 0.0
    for name, p in model[0].named_parameters():
        r = grad64[name]
        if r.abs().max().item() < 1e-9 * gscale:      # mathematically zero (conv bias in front of a BatchNorm)
            assert p.grad.abs().max().item() < 1e-5 * gscale, name
            continue
        e, spread = relerr(p.grad.detach().cpu(), r), relerr(grad32[name], r)
        num += (p.grad.detach().cpu().double() - r).pow(2).sum().item()
        num32 += (grad32[name] - r).pow(2).sum().item()
        den += r.pow(2).sum().item()
        if e > max(4 * spread, 3e-4):
            bad.append((name, e, spread))
    print("MEASURED backbone %dx%d: whole-gradient relative L2 error %.3e (float32 oracle's own %.3e); %d tensors past their bound %s"
          % (h, w, (num / den) ** 0.5, (num32 / den) ** 0.5, len(bad), bad[:4]))
    # whole-gradient relative L2 error: as close to float64 as the float32 CPU reference is (x3)
    assert (num / den) ** 0.5 <= max(3 * (num32 / den) ** 0.5, 1e-4), ((num / den) ** 0.5, (num32 / den) ** 0.5)
    # per tensor: a ReLU whose input is within rounding of zero can flip differently in two float32
    # implementations and moves the few tensors next to it by percents; allow <= 2% such tensors, bounded
    assert len(bad) <= 4 and all(e < 0.25 for _, e, _ in bad), bad[:10]
    # BatchNorm running statistics after the two per-direction updates
    assert relerr(model[0].layer1[1].running_mean.cpu(), bb64.layer1[1].running_mean) < 1e-5
    assert relerr(model[0].layer8[1].running_var.cpu(), bb64.layer8[1].running_var) < 1e-4


def test_backbone_forward_backward_vs_oracle(zeng):
    check_backbone_forward_backward_vs_oracle(zeng, synth.make_pairs(2, seed=3))


def test_head_scenario_vs_golden(zeng, golden):
    """Head only on given perspective fields: loss, MACE, gradient w.r.t. pf against the reference outputs."""
    cfg, model = zeng
    g32, g64 = golden("head_b8_f32"), golden("head_b8_f64")
    head = model[1]
    load_synthetic(head.auxiliary_resnet, 0)
    head.train()
    d = synth.make_head_inputs(8, 7)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta", "pf_hat_12", "pf_hat_21")}
    data["pf_hat_12"].requires_grad_(True)
    data["pf_hat_21"].requires_grad_(True)
    data["choice_12"], data["choice_21"] = cuda(g32["choice_12"], torch.int64), cuda(g32["choice_21"], torch.int64)
    loss, dgt, dh = head(data)
    loss.backward()
    # north_star: fp32 loss within 1e-4 relative of the reference CPU path
    assert abs(loss.item() - g32["loss"]) <= 1e-4 * abs(g32["loss"]), (loss.item(), g32["loss"])
    np.testing.assert_allclose(dh.detach().cpu().numpy(), g32["delta_hat_12"], atol=2e-3)
    from bihome_amd.step import mace
    assert abs(mace(dgt, dh) - g32["mace"]) < 1e-3                      # north_star: MACE within 1e-3
    for k in ("pf_hat_12", "pf_hat_21"):
        got = data[k].grad.cpu().numpy()[:, :, ::4, ::4]
        # the reference's own f32-vs-f64 spread sets the scale of what "equal" means for this gradient
        spread = np.abs(g32["grad_" + k + "_sub"] - g64["grad_" + k + "_sub"]).max()
        tol = max(5 * spread, 1e-4 * np.abs(g64["grad_" + k + "_sub"]).max())
        assert np.abs(got - g64["grad_" + k + "_sub"]).max() <= tol, (k, np.abs(got - g64["grad_" + k + "_sub"]).max(), tol)
    np.testing.assert_allclose(head.auxiliary_resnet.resnet.bn1.running_mean.cpu().numpy(), g32["aux_bn1_running_mean"],
                               rtol=1e-4, atol=1e-5)


def test_zeng_train_step_vs_golden(zeng, golden):
    """One full training step (fwd + bwd + Adam) at the reference's CPU-runnable size (B=8)."""
    from bihome_amd.step import build_optimizer, mace, train_step
    cfg, model = zeng
    g32, g64 = golden("zeng_b8_f32"), golden("zeng_b8_f64")
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    d = synth.make_pairs(8, seed=42)
    losses, maces = [], []
    for it in range(3):
        data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
        data["choice_12"], data["choice_21"] = cuda(g32["choice_12"][it], torch.int64), cuda(g32["choice_21"][it], torch.int64)
        if it == 0:
            model.train()
            opt.zero_grad()
            loss, dgt, dh = model(data)
            pf12 = data["pf_hat_12"].detach().cpu().numpy()
            loss.backward()
            assert relerr(pf12[..., ::8, ::8], g64["pf_hat_12_sub"]) < 2e-4
            # loss of step 0: the reference's own f32-vs-f64 difference is ~1e-5 relative
            assert abs(loss.item() - g64["loss"][0]) <= 1e-4 * abs(g64["loss"][0]), (loss.item(), g64["loss"][0])
            assert abs(mace(dgt, dh) - g64["mace"][0]) < 1e-3
            params = dict(model[0].named_parameters())
            for name in ("layer1.0.weight", "layer4.6.upper_branch.0.weight", "layer8.3.weight", "layer8.3.bias"):
                gn = params[name].grad.double().norm().item()
                ref, spread = g64["gradnorm/" + name], abs(g64["gradnorm/" + name] - g32["gradnorm/" + name])
                assert abs(gn - ref) <= max(5 * spread, 2e-3 * ref), (name, gn, ref, spread)
            opt.step(); sched.step()
            losses.append(loss.item()); maces.append(mace(dgt, dh))
        else:
            loss, dgt, dh = train_step(model, data, opt, sched)
            losses.append(loss.item()); maces.append(mace(dgt, dh))
    # later steps: training from random weights is chaotic (the reference's own f32 and f64 runs differ
    # by |f32-f64|); require agreement within a few of those spreads
    for it in (1, 2):
        spread = abs(g32["mace"][it] - g64["mace"][it])
        assert abs(maces[it] - g64["mace"][it]) <= max(10 * spread, 0.05), (it, maces, g64["mace"])
    assert all(np.isfinite(losses))


def test_training_step_runs_the_plans_the_cpu_planner_makes(zeng):
    """The fusion plans a B=8 training step actually ran with (Program.plans()) are the ones bihome_amd.plan makes on the host for the
    same program and key - what tests/test_plan_cpu.py pins without a GPU is what runs."""
    from bihome_amd import plan as P
    from bihome_amd.step import build_optimizer, train_step
    from test_plan_cpu import _saved_ctx
    cfg, model = zeng
    load_synthetic(model[0], 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    d = synth.make_pairs(8, seed=42)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
    model.train()
    train_step(model, data, opt, sched)
    runner = model[0]._runner
    prog = runner.prog
    used = prog.plans()
    fw, bw = used["last_forward"], used["last_backward"]
    packer = runner.packer_for(torch.device("cuda", torch.cuda.current_device()))
    assert fw is used["forward"][P.forward_key(prog, True, 2, runner.precision, packer, False)]
    assert set(packer.entries) == P.packed_weight_ids(prog)
    want = P.make_forward_plan(prog, True, 2, runner.precision, P.packed_weight_ids(prog))
    for f in P.ForwardPlan.__slots__:
        assert getattr(fw, f) == getattr(want, f), f
    assert len(fw.bn_on_load) == 19 and len(fw.joins) == 6 and fw.bn_pool == {1}          # (as pinned in test_plan_cpu.py)
    ctx = _saved_ctx(prog, (16, 2, 128, 128), 2, True, runner.precision, fw.joins)
    assert bw is used["backward"][P.backward_key(prog, ctx, (16, 2, 128, 128), True)]
    want = P.make_backward_plan(prog, ctx, True)
    for f in P.BackwardPlan.__slots__:
        assert getattr(bw, f) == getattr(want, f), f
    assert bw.fuse_bn and bw.fuse_bias and bw.from_1x1 == {109}


def test_predict_homography_eval_mode(zeng):
    from bihome_amd.step import predict
    cfg, model = zeng
    load_synthetic(model[0], 0)
    bb, head = O.build(cfg)
    load_synthetic(bb, 0)
    bb.eval(); head.eval()
    B = 2
    d = synth.make_pairs(B, seed=9)
    choice = O.sample_choice(128 * 128, B * 128, torch.Generator().manual_seed(3)).reshape(B, 128)
    with torch.no_grad():
        ref, _ = head.predict_homography(bb({k: torch.tensor(d[k]) for k in ("patch_1", "patch_2")}), choice)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2")}
    data["choice"] = choice.cuda()
    got = predict(model, data)
    assert got.shape == (B, 4, 2)
    # eval-mode BN with the initial running statistics gives a wild field; compare relatively
    assert relerr(got.cpu(), ref) < 5e-3


def test_detone_step_vs_golden(golden):
    from bihome_amd.step import build_model
    cfg = configs.get("detone-bihome")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    g32, g64 = golden("detone_b4_f32"), golden("detone_b4_f64")
    d = synth.make_pairs(4, seed=5)
    model.train()
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
    loss, dgt, dh = model(data)
    loss.backward()
    assert abs(loss.item() - g64["loss"]) <= max(3 * abs(g32["loss"] - g64["loss"]), 1e-4 * abs(g64["loss"]))
    np.testing.assert_allclose(dh.detach().cpu().numpy(), g64["delta_hat_12"], rtol=1e-3, atol=1e-4)
    params = dict(model[0].named_parameters())
    for name in ("resnet34.conv1.weight", "resnet34.layer2.0.downsample.0.weight", "resnet34.fc.weight", "resnet34.fc.bias"):
        gn = params[name].grad.double().norm().item()
        ref, spread = g64["gradnorm/" + name], abs(g64["gradnorm/" + name] - g32["gradnorm/" + name])
        assert abs(gn - ref) <= max(5 * spread, 2e-3 * ref), (name, gn, ref, spread)


def test_zeng_bf16_operand_mode_first_step(golden):
    """Mixed-precision conv mode (bf16 MFMA operands, fp32 accumulate and storage): first-step loss and MACE stay
    close to the float64 reference; tolerance = bf16 operand rounding through 59 conv layers (stated, not 1e-4)."""
    from bihome_amd.step import build_model, mace
    cfg = configs.get("zeng-bihome")
    cfg["MODEL"]["BACKBONE"]["PRECISION"] = "bf16"
    cfg["MODEL"]["HEAD"]["PRECISION"] = "bf16"
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    g64 = golden("zeng_b8_f64")
    g32 = golden("zeng_b8_f32")
    d = synth.make_pairs(8, seed=42)
    model.train()
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
    data["choice_12"], data["choice_21"] = cuda(g32["choice_12"][0], torch.int64), cuda(g32["choice_21"][0], torch.int64)
    loss, dgt, dh = model(data)
    loss.backward()
    assert abs(loss.item() - g64["loss"][0]) <= 0.1 * abs(g64["loss"][0]), (loss.item(), g64["loss"][0])
    assert abs(mace(dgt, dh) - g64["mace"][0]) < 0.1
    assert all(torch.isfinite(p.grad).all() for p in model[0].parameters())


def test_checkpoint_compatibility_and_multi_hypothesis_eval(zeng, golden):
    """SURVEY 8(f2,f3): a state dict in the reference's layout (plain OIHW tensors, keys as upstream: here produced
    by the oracle modules, whose keys equal the reference's) loads into the drop-in modules although their conv
    weights live in channels_last memory; and predict_homography with RANSAC_HYPOTHESIS_NO=4 selects the same
    hypothesis index (bit-exact) and delta as the reference run recorded in the golden file."""
    import io
    from bihome_amd.step import build_model
    cfg, model = zeng
    bb, head = O.build(cfg)
    load_synthetic(bb, 3)                      # a different seed than the fixture's model
    load_synthetic(head.auxiliary_resnet, 3)
    buf = io.BytesIO()
    torch.save({"model": torch.nn.Sequential(bb, head).state_dict()}, buf)        # CheckPointer.save layout (checkpoint.py:31-53)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")["model"]
    model2 = build_model(cfg)
    missing = model2.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    for p in model2[0].parameters():
        if p.dim() == 4:
            assert p.permute(0, 2, 3, 1).is_contiguous()          # still kernel layout after loading
    d = synth.make_pairs(2, seed=13)
    bb.double().train()
    ref = bb({k: torch.tensor(d[k], dtype=torch.float64) for k in ("patch_1", "patch_2")})["pf_hat_12"]
    model2.train()
    got = model2[0]({k: cuda(d[k]) for k in ("patch_1", "patch_2")})["pf_hat_12"]
    assert relerr(got.detach().cpu(), ref.detach()) < 1e-4
    rt = model2.state_dict()
    assert set(rt.keys()) == set(sd.keys()) and all(rt[k].shape == sd[k].shape for k in sd)
    # multi-hypothesis eval path
    g = golden("dsac_n4_f32")
    cfg4 = configs.get("zeng-bihome")
    cfg4["MODEL"]["HEAD"].update(RANSAC_HYPOTHESIS_NO=4, POINTS_PER_HYPOTHESIS=16)
    head4 = build_model(cfg4)[1].eval()
    dd = synth.make_head_inputs(8, 11, noise=2.0)
    with torch.no_grad():
        dh, _ = head4.predict_homography({"pf_hat_12": cuda(dd["pf_hat_12"]), "choice": cuda(g["choice"], torch.int64)})
    assert np.array_equal(head4.last["best"].cpu().numpy(), g["best"])
    np.testing.assert_allclose(dh.cpu().numpy(), g["delta_hat"], atol=5e-2)


def test_eval_batchnorm_folding_matches_unfolded(zeng):
    """Inference path: every eval-mode BatchNorm folded into the conv before it (ReLU / residual add in the
    conv epilogue) gives the same perspective field and delta_hat as the unfolded eval pass, after the running
    statistics have moved away from their initial values."""
    from bihome_amd.step import build_optimizer, predict, train_step
    cfg, model = zeng
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    d = synth.make_pairs(4, seed=31)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
    train_step(model, dict(data), opt, sched)          # running statistics != (0, 1)
    g = torch.Generator().manual_seed(2)
    choice = torch.randint(0, 128 * 128, (4, 128), generator=g).cuda()
    runner = model[0]._runner
    outs = {}
    with torch.no_grad():
        for fold in (False, True):
            runner.fold_bn = fold
            batch = dict(data, choice=choice)
            dh = predict(model, batch)
            outs[fold] = (batch["pf_hat_12"].clone(), dh.clone())
    runner.fold_bn = True
    assert len(runner._fold) > 50                       # the Zeng backbone has 54 BatchNorms behind convs
    e_pf, e_dh = relerr(outs[True][0].cpu(), outs[False][0].cpu()), relerr(outs[True][1].cpu(), outs[False][1].cpu())
    print("fold vs unfold: pf %.2e delta_hat %.2e" % (e_pf, e_dh))
    # (folding changes the arithmetic of 54 layers - w * s in fp32 instead of y * s: measured 0.5-2e-4 from run to run)
    assert e_pf < 5e-4
    assert e_dh < 2e-3
    # a training step invalidates the folded weights (running statistics change in place)
    train_step(model, dict(data), opt, sched)
    assert len(runner._fold) == 0


@pytest.mark.parametrize("name,batch,seed", [("zeng-orig", 4, 21), ("detone-orig", 4, 22)])
def test_supervised_orig_configs_vs_golden(golden, name, batch, seed):
    """config/*/zeng-orig, detone-orig (OneLine backbone + NoOpHead + SmoothL1 / MSE loss, train.py:318-322) on the HIP
    path against the reference's own modules: first-step loss, outputs, MACE and gradient norms; the second step's loss
    within the reference's own float32-vs-float64 spread (training from random weights amplifies rounding)."""
    import importlib
    from bihome_amd.step import build_loss, build_model, build_optimizer, mace, predict, train_step
    g32, g64 = golden(name.replace("-", "_") + "_b4_f32"), golden(name.replace("-", "_") + "_b4_f64")
    cfg = configs.get(name)
    model = build_model(cfg)
    assert importlib.import_module("src.heads.NoOpHead").Model is type(model[1])
    load_synthetic(model[0], 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    loss_fn = build_loss(cfg["SOLVER"])
    assert isinstance(loss_fn, torch.nn.Module)
    d = synth.make_pairs(batch, seed=seed, target=True)
    key0 = cfg["MODEL"]["BACKBONE"]["TARGET_KEYS"][0]
    losses = []
    for it in range(2):
        data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta", "target", "corners")}
        loss, dgt, dh = train_step(model, data, opt, sched, loss_fn=loss_fn)
        losses.append(loss.item())
        if it == 0:
            out = data[key0].detach().cpu()
            ref = g64["output0"]
            assert relerr(out[..., ::8, ::8] if out.dim() == 4 else out, ref) < 2e-3
            assert relerr(dh.cpu(), g64["delta_hat0"]) < 2e-3
            assert abs(mace(dgt, dh) - g64["mace"][0]) < 1e-3 * g64["mace"][0]
            names = dict(model[0].named_parameters())
            for k in g64:
                if k.startswith("gradnorm/"):
                    pass            # (gradients are consumed by the optimiser step; norms are pinned through step 2's loss)
    assert abs(losses[0] - g64["loss"][0]) <= 1e-4 * abs(g64["loss"][0])
    spread = abs(g32["loss"][1] - g64["loss"][1])
    assert abs(losses[1] - g64["loss"][1]) <= max(20 * spread, 2e-3 * abs(g64["loss"][1]))
    # inference: predict_homography chain (eval.py:21-28)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta", "target", "corners")}
    dh = predict(model, data)
    assert dh.shape[0] == batch and np.isfinite(mace(data["delta"], dh))
    if name == "zeng-orig":         # NoOpHead._postprocess on an exact field recovers the 4-point offsets
        dh2, H = model[1]._postprocess(cuda(d["target"]))
        assert relerr(dh2.cpu(), d["delta"]) < 1e-3


def test_pretrained_resnet_path_loads_imagenet_layout(tmp_path):
    """PRETRAINED_RESNET = path of a torchvision resnet34 state dict (upstream downloads it): both backbones load it into
    the right modules, keep the kernel (channels_last) weight layout and still run."""
    import importlib
    tv = O._TVResNet34()
    g = torch.Generator().manual_seed(1)
    state = {k: (0.05 * torch.randn(v.shape, generator=g) if v.dtype.is_floating_point else v.clone())
             for k, v in tv.state_dict().items()}
    for k in state:
        if k.endswith("running_var"):
            state[k] = state[k].abs() + 0.5
    path = str(tmp_path / "resnet34.pth")
    torch.save(state, path)
    d = synth.make_pairs(2, seed=3)
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2")}
    cfg = configs.get("zeng-bihome")["MODEL"]["BACKBONE"]
    cfg["PRETRAINED_RESNET"] = path
    bb = importlib.import_module("src.backbones.Rethinking").Model(**cfg).cuda()
    assert torch.equal(bb.state_dict()["layer3.0.lower_branch.0.weight"].cpu(), state["layer2.0.downsample.0.weight"])
    out = bb(dict(data))
    assert torch.isfinite(out["pf_hat_12"]).all()
    cfg = configs.get("detone-bihome")["MODEL"]["BACKBONE"]
    cfg["PRETRAINED_RESNET"] = path
    rb = importlib.import_module("src.backbones.ResNet34").Model(**cfg).cuda()
    assert torch.equal(rb.state_dict()["resnet34.layer4.2.conv2.weight"].cpu(), state["layer4.2.conv2.weight"])
    assert rb.state_dict()["resnet34.conv1.weight"].shape == (64, 2, 7, 7)
    out = rb(dict(data))
    assert torch.isfinite(out["delta_hat_12"]).all()
    with pytest.raises(RuntimeError, match="no network"):
        importlib.import_module("src.backbones.ResNet34").Model(**dict(cfg, PRETRAINED_RESNET=True))


@pytest.mark.parametrize("B,patch", [(3, 128), (1, 128), (5, 64)])
def test_ragged_batches_first_step_vs_oracle(B, patch):
    """Odd / minimal batch sizes and a second patch size: the stacked-direction layout (2B images, 2 statistics groups),
    the odd sub-tile counts of the 3x3 kernel and the fallbacks for small grids against the float64 oracle on the
    same inputs, weights and DSAC indices (first forward + loss + MACE; B = 1 has one image per BatchNorm group)."""
    from bihome_amd.step import build_model, mace
    cfg = configs.get("zeng-bihome")
    cfg["MODEL"]["BACKBONE"]["IMAGE_SIZE"] = patch
    cfg["MODEL"]["HEAD"]["PATCH_SIZE"] = patch
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    bb, head = O.build(cfg)
    load_synthetic(bb, 0)
    load_synthetic(head.auxiliary_resnet, 0)
    bb.double().train(); head.double().train()
    d = synth.make_pairs(B, patch=patch, rho=patch // 4, seed=50 + B)
    g = torch.Generator().manual_seed(B)
    c12 = torch.randint(0, patch * patch, (B, 128), generator=g)
    c21 = torch.randint(0, patch * patch, (B, 128), generator=g)
    ref_data = {k: torch.tensor(d[k], dtype=torch.float64) for k in ("patch_1", "patch_2", "delta")}
    ref_loss, ref_gt, ref_dh = head(bb(ref_data), c12, c21)
    model.train()
    data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
    data["choice_12"], data["choice_21"] = c12.cuda(), c21.cuda()
    loss, dgt, dh = model(data)
    loss.backward()
    torch.cuda.synchronize()
    assert relerr(data["pf_hat_12"].detach().cpu(), ref_data["pf_hat_12"].detach()) < 5e-4
    assert abs(loss.item() - ref_loss.item()) <= 2e-4 * abs(ref_loss.item()) + 1e-6
    assert abs(mace(dgt, dh) - O.mace(ref_gt, ref_dh)) < 2e-3
    assert all(torch.isfinite(p.grad).all() for p in model[0].parameters())


def test_ihome_one_line_vs_golden(golden):
    """iHomE (one-line hinge loss, PerceptualHead.py:465-538) on the HIP path against the reference's own modules: first
    step tight, second step within the reference's float32-vs-float64 spread."""
    from bihome_amd.step import build_model, build_optimizer, mace, train_step
    g32, g64 = golden("zeng_ihome_b4_f32"), golden("zeng_ihome_b4_f64")
    cfg = configs.get("zeng-ihome")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    d = synth.make_pairs(4, seed=31)
    losses, maces = [], []
    for it in range(2):
        data = {k: cuda(d[k]) for k in ("patch_1", "patch_2", "delta")}
        data["choice_12"] = cuda(g32["choice_12"][it], torch.int64)
        loss, dgt, dh = train_step(model, data, opt, sched)
        losses.append(loss.item()); maces.append(mace(dgt, dh))
        if it == 0:
            assert relerr(data["pf_hat_12"].detach().cpu()[..., ::8, ::8], g64["pf_hat_12_sub"]) < 2e-4
            assert relerr(dh.cpu(), g64["delta_hat_12"]) < 1e-3
    assert abs(losses[0] - g64["loss"][0]) <= 2e-4 * abs(g64["loss"][0]), (losses, g64["loss"])
    assert abs(maces[0] - g64["mace"][0]) < 1e-3
    spread = abs(g32["loss"][1] - g64["loss"][1])
    assert abs(losses[1] - g64["loss"][1]) <= max(20 * spread, 2e-3 * abs(g64["loss"][1])), (losses, g64["loss"], g32["loss"])
