"""The reference side of the inference-parity tests, without a GPU: the calibrated oracle is well conditioned (its float32 run stays
within 5e-5 of its float64 run at every BatchNorm), every BatchNorm has a tap and an expectation, `expected_at` is the eval-mode fold
written out from raw parameters, and the operand-rounding model is exact."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import inference_cases as IC
from bihome_amd import net

# rel-L2 of the float32 oracle against the float64 oracle measured when these tests were written: (backbone output, BatchNorm outputs min /
# median / max)
TABLE = {"zeng-bihome": (2.0e-5, 2.6e-7, 4.7e-6, 2.3e-5), "detone-bihome": (2.0e-6, 2.5e-7, 2.3e-6, 6.9e-6),
         "zhang-orig": (1.1e-6, 1.8e-7, 2.1e-6, 5.7e-6)}


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cal = IC.calibrated(name)
            cache[name] = (cal,) + IC.reference(cal, name, IC.pairs(3))
        return cache[name]
    return get


def hip_backbone(cfg):
    """The HIP backbone's module tree and programs on the host (parameter containers and op lists: nothing runs)."""
    import importlib
    bcfg = cfg["MODEL"]["BACKBONE"]
    bb = importlib.import_module("src.backbones." + bcfg["NAME"]).Model(**bcfg)
    stacks = [bb] + [m for m in (getattr(bb, "feature_extractor", None), getattr(bb, "mask_predictor", None))
                     if m is not None and not getattr(m, "fix_mask", False)]
    return bb, [m._build().prog for m in stacks]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_calibrated_oracle_is_well_conditioned(runs, name):
    cal, r64, r32 = runs(name)
    bns = [n for n, m in cal.bb64.named_modules() if isinstance(m, nn.BatchNorm2d) and n in r64.tap]
    e_bn = np.array([IC.rel_l2(r32.tap[n], r64.tap[n]) for n in bns])
    e_out = max(IC.rel_l2(r32.out[k], r64.out[k]) for k in r64.out)
    got = (e_out, e_bn.min(), float(np.median(e_bn)), e_bn.max())
    print("%s: float32 oracle vs float64: output %.2e, BatchNorm outputs %.2e / %.2e / %.2e over %d" % ((name,) + got + (len(bns),)))
    assert len(bns) == IC.BN_COUNT[name]
    # the conditions the GPU bounds rest on, met by the reference alone
    assert e_bn.max() <= 5e-5 and e_out <= 5e-5
    for g, want in zip(got, TABLE[name]):
        assert want / 2 <= g <= want * 2, (got, TABLE[name])
    # statistics really moved away from (0, 1), and the two dtypes carry the same weights
    bn = dict(cal.bb64.named_modules())[bns[len(bns) // 2]]
    assert (bn.running_mean.abs() > 1e-3).any() and ((bn.running_var - 1).abs() > 1e-3).any() and bn.momentum == 0.1
    assert not cal.bb64.training and not cal.bb32.training
    assert all(torch.equal(v.float(), cal.bb32.state_dict()[k].float()) for k, v in cal.sd.items())


@pytest.mark.parametrize("name", sorted(IC.BN_COUNT))
def test_every_batchnorm_has_a_tap_and_an_expectation(name):
    cal = IC.calibrated(name)
    batch = IC.pairs(1)
    r = IC.oracle_run(cal, name, {k: v[:, :, :32, :32] for k, v in batch.items()})         # (fully convolutional: a small map is enough for a census)
    bb, progs = hip_backbone(cal.cfg)
    assert set(bb.state_dict()) == set(cal.sd)
    names = {m: n for n, m in bb.named_modules()}
    oracle_bns = {n for n, m in cal.bb64.named_modules() if isinstance(m, nn.BatchNorm2d)}
    ran = {n for n in oracle_bns if n in r.tap}
    idle = oracle_bns - ran
    assert len(ran) == IC.BN_COUNT[name]
    assert all(n.startswith("mask_predictor.") for n in idle) and (not idle or cal.bb64.mask_predictor.fix_mask)
    covered = set()
    for prog in progs:
        for op in prog.ops:
            if op.kind in ("bn", "tail"):
                want = IC.expected_at(op, r.tap, names)
                assert torch.is_tensor(want) and torch.isfinite(want).all()
                covered.add(names[op.mod[1]] if op.kind == "tail" else names[op.mod])
    assert covered == ran


def test_expected_at_is_the_fold_written_out():
    """conv -> BN -> ReLU, residual joins with and without a lower branch, ConvTranspose2d -> BN: the hooks' value at every BatchNorm
    position equals the value recomputed from raw parameters and from folded weights w s, b s + t, to 1e-12 - the definition net._folded
    has to meet, restated independently of it."""
    tiny = IC.tiny_net()
    prog = net.Program()
    prog.sequential(0, tiny)
    x = torch.randn(2, 2, 12, 20, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    seen, handles = {}, []
    for name, m in tiny.named_modules():
        if isinstance(m, (nn.BatchNorm2d, IC.O._Res)):
            handles.append(m.register_forward_hook(lambda mod, a, out, name=name: seen.__setitem__(name, out.detach())))
    with torch.no_grad():
        tiny(x)
    for h in handles:
        h.remove()
    names = {m: n for n, m in tiny.named_modules()}
    raw, folded = IC.restate(prog, x, False), IC.restate(prog, x, True)
    bn_ops = [i for i, op in enumerate(prog.ops) if op.kind == "bn"]
    assert len(bn_ops) == 9 and sorted(raw) == bn_ops == sorted(folded)
    kinds = set()
    for i in bn_ops:
        op = prog.ops[i]
        want = IC.expected_at(op, seen, names)
        scale = want.abs().max().item()
        for got in (raw[i], folded[i]):
            assert (got - want).abs().max().item() <= 1e-12 * max(scale, 1.0), (names[op.mod], (got - want).abs().max().item())
        producer = next(o for o in prog.ops if o.dst == op.src)
        kinds.add((type(producer.mod).__name__, producer.mod.bias is not None, op.res is not None, op.relu))
    # every arm is present: a biased conv, a bias-free ConvTranspose2d, plain / ReLU / residual positions
    assert {("Conv2d", True, False, True), ("ConvTranspose2d", False, False, False), ("Conv2d", False, True, True),
            ("Conv2d", False, False, False)} <= kinds


def test_fold_definition_catches_the_wrong_axis_and_eps():
    """The restatement has teeth: scaling a ConvTranspose2d along its input axis, or leaving eps out, moves the result far past 1e-12."""
    tiny = IC.tiny_net()
    prog = net.Program()
    prog.sequential(0, tiny)
    x = torch.randn(1, 2, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    good = IC.restate(prog, x, True)
    lower_bn = tiny[5].lower_branch[1]
    i = next(j for j, op in enumerate(prog.ops) if op.mod is lower_bn)
    convt = tiny[5].lower_branch[0]
    assert convt.in_channels != convt.out_channels                        # (else the wrong axis would not even raise or differ in shape)
    s, t = IC.bn_coefficients(lower_bn)
    with torch.no_grad():
        src = IC.restate(prog, x, False)[i - 2]                           # the unit's input: the strided unit's stored output
        wrong_eps = IC._conv(convt, src, convt.weight * (lower_bn.weight / lower_bn.running_var.sqrt()).view(1, -1, 1, 1), t)
    assert (wrong_eps - good[i]).abs().max().item() > 1e-7
    with pytest.raises(RuntimeError):
        convt.weight * s.view(-1, 1, 1, 1)                                # 8 scales along the 16-channel input axis


def test_round_mantissa_is_exact():
    r = IC.round_mantissa
    # on the grid: unchanged (bfloat16 values through 8 bits, float32 values through 24)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g) * torch.tensor(2.0) ** torch.randint(-20, 20, (4096,), generator=g)
    b = x.bfloat16().double()
    assert torch.equal(r(b, 8), b) and torch.equal(r(x.double(), 24), x.double())
    assert torch.equal(r(torch.zeros(3), 8), torch.zeros(3))
    # off the grid: torch's own round-to-nearest-even conversion
    assert torch.equal(r(x.double(), 8), x.bfloat16().double())
    xd = torch.randn(4096, generator=g, dtype=torch.float64)
    assert torch.equal(r(xd, 24), xd.float().double())
    # ties go to even: 1 + k 2^-8 lies midway between two 8-bit neighbours for odd k
    ties = torch.tensor([1 + 1 / 256, 1 + 3 / 256, -(1 + 1 / 256), 2 + 2 / 256, 2 + 6 / 256], dtype=torch.float64)
    want = torch.tensor([1.0, 1 + 4 / 256, -1.0, 2.0, 2 + 8 / 256], dtype=torch.float64)
    assert torch.equal(r(ties, 8), want)
    # 16 bits: at most half a unit in the 16th place, and idempotent
    y = r(xd, 16)
    assert ((y - xd).abs() <= xd.abs() * 2.0 ** -16).all() and torch.equal(r(y, 16), y)
    assert r(x, 8).dtype == x.dtype


def test_rounded_operands_round_inputs_and_weights_and_restore():
    tiny = IC.tiny_net()
    x = torch.randn(1, 2, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    before = {k: v.clone() for k, v in tiny.state_dict().items()}
    seen = []
    convs = [m for m in tiny.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    handles = [m.register_forward_hook(lambda mod, a, out: seen.append((a[0].clone(), mod.weight.detach().clone()))) for m in convs]
    with torch.no_grad():
        exact = tiny(x)
        seen.clear()
        with IC.rounded_operands(tiny, 8):
            rounded = tiny(x)
    for h in handles:
        h.remove()
    assert len(seen) == len(convs) == 10
    for a, w in seen:
        assert torch.equal(IC.round_mantissa(a, 8), a) and torch.equal(IC.round_mantissa(w, 8), w)
    assert all(torch.equal(v, before[k]) for k, v in tiny.state_dict().items())
    e = IC.rel_l2(rounded, exact)
    assert 2.0 ** -11 < e < 2.0 ** -5, e                                   # bfloat16 operands: a unit roundoff of 2^-9 through ten layers
    with torch.no_grad():
        assert torch.equal(tiny(x), exact)
        # restricted to one conv: only that one sees rounded operands, and the result moves less
        seen.clear()
        handles = [m.register_forward_hook(lambda mod, a, out: seen.append((mod, a[0].clone(), mod.weight.detach().clone()))) for m in convs]
        with IC.rounded_operands(tiny, 8, only={"3.upper_branch.3"}):
            one = tiny(x)
        for h in handles:
            h.remove()
    on_grid = [m for m, a, w in seen if torch.equal(IC.round_mantissa(a, 8), a) and torch.equal(IC.round_mantissa(w, 8), w)]
    assert on_grid == [tiny[3].upper_branch[3]] and 0 < IC.rel_l2(one, exact) < e
    with pytest.raises(AssertionError):
        with IC.rounded_operands(tiny, 8, only={"3.upper_branch.4"}):        # a BatchNorm: no conv of that name
            pass


def test_bf16_operand_rule_names_the_convs_behind_the_vector_loader():
    for name, count, fp32 in (("zeng-bihome", 56, {"layer1.0", "layer8.0", "layer8.3"}), ("detone-bihome", 36, {"resnet34.conv1"})):
        cal = IC.calibrated(name)
        convs = {n for n, m in cal.bb32.named_modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear))}
        rounded = IC.bf16_operand_convs(cal.bb32, name)
        assert convs - rounded == fp32 and len(rounded) == count, (name, len(rounded), sorted(convs - rounded))
