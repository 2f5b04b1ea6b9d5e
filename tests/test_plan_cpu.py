"""Fusion planning (bihome_amd/plan.py) without a GPU: the planners against the in-line planning code they were split out of (kept
below, unchanged, as _legacy_forward_plan / _legacy_backward_plan), readable pins of the Zeng backbone's training plan, and the program
index on a hand-built program."""
import itertools
import types

import pytest
import torch.nn as nn

from bihome_amd import configs, net, plan as P
from bihome_amd import kernels as K


# -----------------------------------------------------------------------------------------------
# the planning blocks of run_forward / run_backward as they stood before plan.py (only the names of the inputs are adapted)
# -----------------------------------------------------------------------------------------------
def _legacy_forward_plan(prog, training, groups, precision, packed_ids, fold=False):
    packer = None if packed_ids is None else types.SimpleNamespace(entries=packed_ids)
    nrec = 0
    if int(precision) == K.F16X2:
        nrec = max(1, sum(1 for op in prog.ops if op.kind == "bn" or (op.kind == "conv" and isinstance(op.mod, nn.ConvTranspose2d))))
    bn_off, total = {}, 0
    for i, op in enumerate(prog.ops):
        if op.kind == "bn":
            bn_off[i] = total
            total += K.bn_stats_doubles(groups, op.mod.num_features)
    consumer = None
    fused_stats = {}                                      # conv op index -> bn op index
    if training:
        users = {}
        for op in prog.ops:
            users[op.src] = users.get(op.src, 0) + 1
            if op.res is not None:
                users[op.res] = users.get(op.res, 0) + 1
        producer = {op.dst: j for j, op in enumerate(prog.ops)}
        for i, op in enumerate(prog.ops):
            j = producer.get(op.src)
            if (op.kind == "bn" and j is not None and prog.ops[j].kind == "conv" and users.get(op.src, 0) == 1
                    and not prog.ops[j].extra["out_nchw"] and prog.ops[j].mod.weight.dim() == 4):
                fused_stats[j] = i
    bn_on_load = set()
    bn_on_load_1x1 = set()
    if training and groups <= 2 and int(precision) != 1:      # (not the bf16-operand mode)
        consumer_ = {}
        for j, op in enumerate(prog.ops):
            consumer_.setdefault(op.src, j)
        fused_bn_ = set(fused_stats.values())
        for i, op in enumerate(prog.ops):
            j = consumer_.get(op.dst)
            if (op.kind == "bn" and op.res is None and i in fused_bn_ and users.get(op.dst, 0) == 1 and j is not None
                    and prog.ops[j].kind == "conv" and prog.ops[j].src == op.dst and prog.ops[j].extra["weight_fn"] is None
                    and not prog.ops[j].extra["in_nchw"] and not prog.ops[j].extra["out_nchw"] and isinstance(prog.ops[j].mod, nn.Conv2d)
                    and prog.ops[j].mod.kernel_size == (1, 1) and prog.ops[j].mod.stride == (1, 1) and prog.ops[j].mod.padding == (0, 0)
                    and prog.ops[j].mod.in_channels % 32 == 0 and prog.ops[j].mod.out_channels % 4 == 0
                    and min(prog.ops[j].mod.in_channels, prog.ops[j].mod.out_channels) <= 32 and prog.ops[j].mod.weight.requires_grad):
                bn_on_load_1x1.add(i)
    if training and packer is not None and int(precision) in K.SPLIT_PIECES:
        consumer = {}
        for j, op in enumerate(prog.ops):
            consumer.setdefault(op.src, j)
        fused_bn = set(fused_stats.values())
        for i, op in enumerate(prog.ops):
            j = consumer.get(op.dst)
            if (op.kind == "bn" and op.res is None and i in fused_bn and users.get(op.dst, 0) == 1 and j is not None
                    and prog.ops[j].kind == "conv" and prog.ops[j].src == op.dst and prog.ops[j].extra["weight_fn"] is None
                    and not prog.ops[j].extra["in_nchw"] and id(prog.ops[j].mod.weight) in packer.entries
                    and groups * op.mod.num_features * 8 <= 4096):
                bn_on_load.add(i)
    joins = {}                                            # join bn op index -> lower bn op index
    if training:
        producer_ = {op.dst: j for j, op in enumerate(prog.ops)}
        for i, op in enumerate(prog.ops):
            j = producer_.get(op.res) if (op.kind == "bn" and op.res is not None) else None
            if (j is not None and prog.ops[j].kind == "bn" and prog.ops[j].res is None and not prog.ops[j].relu
                    and users.get(op.res, 0) == 1 and j not in bn_on_load and i not in bn_on_load
                    and op.mod.num_features == prog.ops[j].mod.num_features and op.mod.num_features % 4 == 0
                    and op.mod.weight is not None and prog.ops[j].mod.weight is not None):
                joins[i] = j
    join_lower = set(joins.values())
    folded = {}                                           # bn op index -> conv op index (conv deferred to the bn's position)
    if fold:
        users = {}
        for op in prog.ops:
            users[op.src] = users.get(op.src, 0) + 1
            if op.res is not None:
                users[op.res] = users.get(op.res, 0) + 1
        producer = {op.dst: j for j, op in enumerate(prog.ops)}
        for i, op in enumerate(prog.ops):
            j = producer.get(op.src)
            if (op.kind == "bn" and j is not None and prog.ops[j].kind == "conv" and users.get(op.src, 0) == 1
                    and not prog.ops[j].extra["out_nchw"]):
                folded[i] = j
    deferred = set(folded.values())
    # the static clauses of the BatchNorm -> MaxPool pairing, which the execution loop evaluated per BatchNorm per call
    bn_pool = set()
    for i, op in enumerate(prog.ops):
        if op.kind != "bn":
            continue
        m = op.mod
        nxt = prog.ops[i + 1] if i + 1 < len(prog.ops) else None
        if (op.res is None and nxt is not None and nxt.kind == "maxpool" and nxt.src == op.dst
                and m.num_features % 4 == 0 and m.num_features > 1 and sum(1 for o_ in prog.ops if o_.src == op.dst or o_.res == op.dst) == 1):
            bn_pool.add(i)
    return dict(fused_stats=fused_stats, bn_on_load=bn_on_load, bn_on_load_1x1=bn_on_load_1x1, joins=joins, join_lower=join_lower,
                consumer=consumer, bn_pool=bn_pool, folded=folded, deferred=deferred, bn_off=bn_off, total=total, nrec=nrec)


_FROM_1X1_KC = (16,)


def _legacy_backward_plan(prog, ctx, want_wgrad):
    consumed_by = {}
    for op in prog.ops:
        consumed_by.setdefault(op.src, 0)
        consumed_by[op.src] += 1
        if op.res is not None:
            consumed_by[op.res] = consumed_by.get(op.res, 0) + 1
    fuse_bn = {}                                          # conv op index -> bn op index
    if ctx.training:
        producer = {op.dst: j for j, op in enumerate(prog.ops)}
        last_consumer = {}
        for j, op in enumerate(prog.ops):                 # the lowest-index consumer is processed last
            for sl in (op.src, op.res):
                if sl is not None and sl not in last_consumer:
                    last_consumer[sl] = j
        for j, op in enumerate(prog.ops):
            b = producer.get(op.src)
            if (op.kind == "conv" and b is not None and prog.ops[b].kind == "bn" and last_consumer.get(op.src) == j
                    and j in ctx.descs and ctx.descs[j].bh_reduce_ok and ctx.descs[j].N % ctx.groups == 0 and b not in ctx.joined):
                fuse_bn[j] = b
    fuse_bias = {}                                        # conv op index -> producer op index
    if want_wgrad:
        producer = {op.dst: j for j, op in enumerate(prog.ops)}
        for j, op in enumerate(prog.ops):
            p = producer.get(op.src)
            if (op.kind == "conv" and j not in fuse_bn and p is not None and prog.ops[p].kind == "conv" and consumed_by.get(op.src, 0) == 1
                    and j in ctx.descs and p in ctx.descs and ctx.descs[j].bh_reduce_ok):
                pm = prog.ops[p].mod
                if pm.bias is not None and pm.bias.requires_grad and pm.weight.requires_grad and prog.ops[p].extra["weight_fn"] is None:
                    fuse_bias[j] = p
    from_1x1 = set()
    if ctx.training:
        producer_ = {op.dst: j for j, op in enumerate(prog.ops)}
        for j, op in enumerate(prog.ops):
            b = producer_.get(op.src)
            m_ = op.mod
            if (op.kind == "conv" and b is not None and prog.ops[b].kind == "bn" and prog.ops[b].res is None and b not in ctx.joined
                    and consumed_by.get(op.src, 0) == 1 and j not in fuse_bn and isinstance(m_, nn.Conv2d) and m_.kernel_size == (1, 1)
                    and m_.stride == (1, 1) and m_.padding == (0, 0) and op.extra["weight_fn"] is None and m_.out_channels in _FROM_1X1_KC
                    and prog.ops[b].mod.num_features % 4 == 0 and 256 % (prog.ops[b].mod.num_features // 4) == 0
                    and not op.extra["in_nchw"] and not op.extra["out_nchw"]):
                from_1x1.add(j)
    red_off, total = {}, 0
    bias_off = {}
    for j, p in fuse_bias.items():
        bias_off[p] = total
        total += K.bn_stats_doubles(1, ctx.descs[j].Ci)
    for b in fuse_bn.values():
        red_off[b] = total
        total += K.bn_stats_doubles(ctx.groups, prog.ops[b].mod.num_features)
    nrec = max(1, sum(1 for op in prog.ops if op.kind == "bn")) if getattr(ctx, "precision", 0) == K.F16X2 else 0
    return dict(consumed_by=consumed_by, fuse_bn=fuse_bn, fuse_bias=fuse_bias, from_1x1=from_1x1, red_off=red_off, bias_off=bias_off,
                total=total, nrec=nrec)


# -----------------------------------------------------------------------------------------------
# programs and host-side stand-ins for what a forward pass saves
# -----------------------------------------------------------------------------------------------
def _program(name):
    """(program, input shape per stacked image count N) of a real model, built on the CPU."""
    if name == "zeng-bihome":
        from bihome_amd.backbones.Rethinking import Model
        return Model(**configs.get(name)["MODEL"]["BACKBONE"])._build().prog, lambda N: (N, 2, 128, 128)
    if name == "detone-bihome":
        from bihome_amd.backbones.ResNet34 import Model
        return Model(**configs.get(name)["MODEL"]["BACKBONE"])._build().prog, lambda N: (N, 2, 128, 128)
    from bihome_amd.heads.PerceptualHead import AuxiliaryResnet          # the frozen ResNet-34 extractor, one-channel program
    return AuxiliaryResnet(**configs.get("zeng-bihome")["MODEL"]["HEAD"])._runner(1).prog, lambda N: (N, 128, 128, 1)


PROGRAMS = ("zeng-bihome", "detone-bihome", "extractor")


def _eligible_ids(prog):
    """Weights a Runner's WeightPacker holds (the eligibility test of Runner.packer_for as it stood, device aside)."""
    ids = set()
    for op in prog.ops:
        m = op.mod
        if (op.kind == "conv" and isinstance(m, nn.Conv2d) and op.extra["weight_fn"] is None and m.kernel_size == (3, 3)
                and m.stride == (1, 1) and m.padding == (1, 1) and m.in_channels % 32 == 0 and m.out_channels % 32 == 0):
            ids.add(id(m.weight))
    return ids


def _saved_ctx(prog, x_shape, groups, training, precision, joins):
    """A net.Ctx as run_forward leaves it, as far as the backward planner reads it: conv descriptors from the real _conv_geometry
    (shapes propagated with K.conv_out_shape), the joins that the forward forms when the batch divides into the groups."""
    ctx = net.Ctx()
    ctx.groups, ctx.training, ctx.precision = groups, training, int(precision)
    shapes = {0: tuple(x_shape)}
    for i, op in enumerate(prog.ops):
        s = shapes[op.src]
        if op.kind == "conv":
            d = net._conv_geometry(op.mod, s, op.extra["in_nchw"], op.extra["out_nchw"], precision)
            ctx.descs[i] = d
            s = K.conv_out_shape(d)
        elif op.kind == "maxpool":                        # MaxPool2d(3, 2, 1)
            s = (s[0], (s[1] - 1) // 2 + 1, (s[2] - 1) // 2 + 1, s[3])
        elif op.kind == "gap":
            s = (s[0], 1, 1, s[3])
        elif op.kind == "tail":
            s = (s[0], op.mod[2].out_channels, s[1], s[2])
        elif op.kind == "bn" and i in joins and s[0] % groups == 0:
            ctx.joined[i] = joins[i]
        shapes[op.dst] = s
    return ctx


def _resolve(precision, packed_ids):
    """run_forward's downgrade of the fp16-piece arithmetic without an fp16 packer (before the plan key is formed)."""
    return 2 if (precision == K.F16X2 and packed_ids is None) else precision


def _assert_same(new, legacy, where):
    for f, want in legacy.items():
        assert getattr(new, f) == want, (where, f)


# -----------------------------------------------------------------------------------------------
# 1. parity with the in-line planner
# -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=PROGRAMS)
def program(request):
    return (request.param,) + _program(request.param)


def _parity(prog, x_shape_of, name):
    assert P.packed_weight_ids(prog) == _eligible_ids(prog)
    n = 0
    for training, groups, precision, packed in itertools.product((True, False), (1, 2, 4), (0, 1, 2, 3, 4), (False, True)):
        packed_ids = _eligible_ids(prog) if packed else None
        prec = _resolve(precision, packed_ids)
        where = (name, training, groups, precision, packed)
        fw = P.make_forward_plan(prog, training, groups, prec, packed_ids)
        legacy = _legacy_forward_plan(prog, training, groups, prec, packed_ids)
        _assert_same(fw, legacy, where)
        if not training:                                  # the BatchNorm-folded inference pass (never with a packer: NetFunction._forward)
            fprec = _resolve(precision, None)
            _assert_same(P.make_forward_plan(prog, training, groups, fprec, None, fold=True),
                         _legacy_forward_plan(prog, training, groups, fprec, None, fold=True), where + ("fold",))
        for N in (128, 128 + 1):                          # 64 pairs stacked in both directions; a batch that no group count divides
            if N % groups and groups == 1:
                continue
            ctx = _saved_ctx(prog, x_shape_of(N), groups, training, prec, legacy["joins"])
            for want_wgrad in (True, False):
                _assert_same(P.make_backward_plan(prog, ctx, want_wgrad), _legacy_backward_plan(prog, ctx, want_wgrad),
                             where + (N, want_wgrad))
                n += 1
    return n


def test_planners_match_inline_planning(program):
    name, prog, x_shape_of = program
    assert _parity(prog, x_shape_of, name) >= 2 * 3 * 5 * 2 * 2


def test_planners_match_with_a_frozen_conv():
    prog, x_shape_of = _program("zeng-bihome")
    convs = [op for op in prog.ops if op.kind == "conv"]
    # a decoder unit's 1x1 conv (bn_on_load_1x1 reads its flag) and a biased transposed conv (fuse_bias reads its flags)
    frozen = [next(op for op in convs if isinstance(op.mod, nn.Conv2d) and op.mod.kernel_size == (1, 1) and op.mod.in_channels == 32),
              next(op for op in convs if isinstance(op.mod, nn.ConvTranspose2d) and op.mod.bias is not None)]
    for op in frozen:
        op.mod.weight.requires_grad = False
        try:
            assert at_least_one_field_moves(prog, op)
            _parity(prog, x_shape_of, "zeng-bihome/frozen")
        finally:
            op.mod.weight.requires_grad = True


def at_least_one_field_moves(prog, op):
    """Freezing `op` changes the plan (so the parity above is not vacuous): the flag is read by bn_on_load_1x1 / fuse_bias."""
    op.mod.weight.requires_grad = True
    fw1 = _legacy_forward_plan(prog, True, 2, 4, _eligible_ids(prog))
    bw1 = _legacy_backward_plan(prog, _saved_ctx(prog, (128, 2, 128, 128), 2, True, 4, fw1["joins"]), True)
    op.mod.weight.requires_grad = False
    fw0 = _legacy_forward_plan(prog, True, 2, 4, _eligible_ids(prog))
    bw0 = _legacy_backward_plan(prog, _saved_ctx(prog, (128, 2, 128, 128), 2, True, 4, fw0["joins"]), True)
    return fw0 != fw1 or bw0 != bw1


# -----------------------------------------------------------------------------------------------
# 2. readable pins: zeng-bihome, training, two statistics groups, default arithmetic, packed weights
# -----------------------------------------------------------------------------------------------
# written down from the output of _legacy_forward_plan / _legacy_backward_plan for this configuration (op indices of the fused-tail program)
PINS = {
    "forward": {"fused_stats": 53, "bn_on_load": 19, "bn_on_load_1x1": 2, "joins": 6, "join_lower": 6, "consumer": 106, "bn_pool": 1,
                "folded": 0, "deferred": 0, "bn_off": 53, "total": 446464, "nrec": 61},
    "backward": {"consumed_by": 112, "fuse_bn": 30, "fuse_bias": 4, "from_1x1": 1, "red_off": 30, "bias_off": 4, "total": 304128,
                 "nrec": 53},
    "bn_on_load_1x1": [97, 108],
    "from_1x1": [109],
    "joins": [(20, 16), (38, 34), (65, 60), (84, 79), (99, 94), (110, 105)],
}


def test_zeng_training_plan_pins():
    from bihome_amd.backbones.Rethinking import Model
    model = Model(**configs.get("zeng-bihome")["MODEL"]["BACKBONE"])
    runner = model._build()
    prog, ops = runner.prog, runner.prog.ops
    assert runner.precision == K.F16X2
    at = {id(op.mod): i for i, op in enumerate(ops) if op.kind in ("conv", "bn")}
    fw = P.make_forward_plan(prog, True, 2, runner.precision, P.packed_weight_ids(prog))
    ctx = _saved_ctx(prog, (128, 2, 128, 128), 2, True, runner.precision, fw.joins)
    bw = P.make_backward_plan(prog, ctx, True)
    # sizes, as the in-line planner of the parent revision gives them
    assert PINS["forward"] == {f: (getattr(fw, f) if isinstance(getattr(fw, f), int) else len(getattr(fw, f)))
                               for f in PINS["forward"]}
    assert PINS["backward"] == {f: (getattr(bw, f) if isinstance(getattr(bw, f), int) else len(getattr(bw, f)))
                                for f in PINS["backward"]}
    # the stem's BatchNorm, followed by MaxPool2d(3, 2, 1)
    assert fw.bn_pool == {at[id(model.layer1[1])]}
    # the inner BatchNorm of the first residual unit: applied on load by the unit's second 3x3 conv
    unit = model.layer2[0]
    assert at[id(unit.upper_branch[1])] in fw.bn_on_load
    # a strided unit's downsample BatchNorm is applied inside the join with the upper branch's last BatchNorm
    strided = model.layer3[0]
    assert fw.joins[at[id(strided.upper_branch[-1])]] == at[id(strided.lower_branch[-1])]
    assert at[id(strided.lower_branch[-1])] in fw.join_lower
    # the decoder unit with 16 output channels (layer7): its 1x1 conv leaves the dgrad to the BatchNorm in front
    one_by_one = [i for i, op in enumerate(ops) if op.kind == "conv" and isinstance(op.mod, nn.Conv2d)
                  and op.mod.kernel_size == (1, 1) and op.mod.out_channels == 16]
    assert one_by_one and set(one_by_one) & bw.from_1x1
    assert PINS["from_1x1"] == sorted(bw.from_1x1) and PINS["bn_on_load_1x1"] == sorted(fw.bn_on_load_1x1)
    assert PINS["joins"] == sorted(fw.joins.items())




# -----------------------------------------------------------------------------------------------
# 3. the index
# -----------------------------------------------------------------------------------------------
def test_program_index_by_hand():
    prog = net.Program()
    c, b = nn.Conv2d(4, 4, 3, padding=1), nn.BatchNorm2d(4)
    s1 = prog.conv(0, c)                       # op 0: slot 0 -> 1
    s2 = prog.bn(s1, b, relu=True)             # op 1: 1 -> 2
    s3 = prog.conv(s2, c)                      # op 2: 2 -> 3
    s4 = prog.bn(s3, b, relu=True, res=s2)     # op 3: 3 (+ residual 2) -> 4
    s5 = prog.maxpool(s4)                      # op 4: 4 -> 5
    ix = prog.index()
    assert (s1, s2, s3, s4, s5) == (1, 2, 3, 4, 5) and ix.nops == 5
    assert ix.producer == {1: 0, 2: 1, 3: 2, 4: 3, 5: 4}
    assert ix.consumers == {0: [0], 1: [1], 2: [2, 3], 3: [3], 4: [4]}
    assert ix.users == {0: 1, 1: 1, 2: 2, 3: 1, 4: 1}
    assert ix.consumer == {0: 0, 1: 1, 2: 2, 3: 3, 4: 4}          # by src only: the residual read of slot 2 by op 3 does not count
    assert ix.last_consumer == {0: 0, 1: 1, 2: 2, 3: 3, 4: 4}
    assert prog.index() is ix
    # a program is not extended after it ran: if it is, the index and the plans made from the shorter list go
    prog.fw_plans["stale"] = object()
    prog.gap(s5)
    assert prog.index() is not ix and prog.index().nops == 6 and not prog.fw_plans
