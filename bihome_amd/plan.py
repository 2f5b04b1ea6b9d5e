"""Fusion planning for the conv-stack executor (net.py): which launches of a Program are merged into their neighbours.

Everything here is host logic over the op list, module hyper-parameters and what the library answers for a conv descriptor - no
tensor is touched, so a plan can be made and inspected without a GPU (tests/test_plan_cpu.py).  net.run_forward / run_backward fetch a
ForwardPlan / BackwardPlan through forward_plan() / backward_plan(), which keep them on the program: planning costs ~0.4 ms of host
time per step, of a host that has ~6.6 ms of enqueueing to do per 12 ms step.

A new fusion is a new plan_*() function, a field of the plan it belongs to and the arm of the executor that reads it.
"""
import torch.nn as nn

from . import kernels as K


class ProgramIndex:
    """Who writes and who reads each slot of a Program (made once per program: Program.index())."""
    __slots__ = ("nops", "producer", "consumers", "users", "consumer", "last_consumer")

    def __init__(self, ops):
        self.nops = len(ops)
        self.producer = {op.dst: j for j, op in enumerate(ops)}       # slot -> op index
        self.consumers = {}                                           # slot -> op indices reading it as src or res, ascending
        self.consumer = {}                                            # slot -> first op reading it as src (residual reads do not count)
        for j, op in enumerate(ops):
            self.consumers.setdefault(op.src, []).append(j)
            if op.res is not None:
                self.consumers.setdefault(op.res, []).append(j)
            self.consumer.setdefault(op.src, j)
        self.users = {s: len(v) for s, v in self.consumers.items()}   # slot -> number of reads
        self.last_consumer = {s: v[0] for s, v in self.consumers.items()}   # the lowest-index reader is processed last in backward order


def packs_weight(op, device=None):
    """A conv op whose weight gets fragment-ordered copies (kernels.WeightPacker, read by the halo-tiled 3x3 kernel)."""
    m = op.mod
    return (op.kind == "conv" and isinstance(m, nn.Conv2d) and op.extra["weight_fn"] is None and m.kernel_size == (3, 3)
            and m.stride == (1, 1) and m.padding == (1, 1) and m.in_channels % 32 == 0 and m.out_channels % 32 == 0
            and (device is None or m.weight.device == device))


def packed_weight_ids(prog):
    """id() of every weight of `prog` that a WeightPacker would hold (what the planner needs of a packer built for this program)."""
    return {id(op.mod.weight) for op in prog.ops if packs_weight(op)}


# -----------------------------------------------------------------------------------------------
# forward
# -----------------------------------------------------------------------------------------------
class ForwardPlan:
    __slots__ = ("nops", "fused_stats", "bn_on_load", "bn_on_load_1x1", "joins", "join_lower", "consumer", "bn_pool", "folded", "deferred",
                 "bn_off", "total", "nrec")


def forward_key(prog, training, groups, precision, packer, fold):
    """What can differ between two forward walks of one program: the mode, the statistics groups, the arithmetic, the weight packer (named
    by its serial number, not by id(): an id can be reused by another packer after garbage collection), which conv weights train, and
    whether BatchNorms are folded into their convs (inference only)."""
    return (bool(training), int(groups), int(precision), packer.serial if packer is not None else 0,
            len(packer.entries) if packer is not None else 0, bool(packer.f16) if packer is not None else False,
            tuple(op.mod.weight.requires_grad for op in prog.ops if op.kind == "conv"), bool(fold))


def plan_fused_stats(prog, ix, training):
    """conv op index -> bn op index: a conv whose only consumer is a training-mode BatchNorm accumulates that layer's statistics in its
    own epilogue."""
    fused_stats = {}
    if training:
        ops = prog.ops
        for i, op in enumerate(ops):
            j = ix.producer.get(op.src)
            if (op.kind == "bn" and j is not None and ops[j].kind == "conv" and ix.users.get(op.src, 0) == 1
                    and not ops[j].extra["out_nchw"] and ops[j].mod.weight.dim() == 4 and not ops[j].relu):
                fused_stats[j] = i
    return fused_stats


def plan_bn_on_load_1x1(prog, ix, training, groups, precision, fused_stats):
    """BatchNorm-on-load (see plan_bn_on_load) for a 1x1 / stride-1 conv consumer with <= 32 channels on one side (the 1x1 conv of the
    decoder units behind BatchNorm + ReLU at 64 x 64 and 128 x 128): generic forward kernel and small-channel weight-gradient kernel
    transform on load."""
    out = set()
    if training and groups <= 2 and int(precision) != 1:      # (not the bf16-operand mode)
        ops = prog.ops
        fused_bn = set(fused_stats.values())
        for i, op in enumerate(ops):
            j = ix.consumer.get(op.dst)
            if (op.kind == "bn" and op.res is None and i in fused_bn and ix.users.get(op.dst, 0) == 1 and j is not None
                    and ops[j].kind == "conv" and ops[j].src == op.dst and ops[j].extra["weight_fn"] is None
                    and not ops[j].extra["in_nchw"] and not ops[j].extra["out_nchw"] and isinstance(ops[j].mod, nn.Conv2d)
                    and ops[j].mod.kernel_size == (1, 1) and ops[j].mod.stride == (1, 1) and ops[j].mod.padding == (0, 0)
                    and ops[j].mod.in_channels % 32 == 0 and ops[j].mod.out_channels % 4 == 0
                    and min(ops[j].mod.in_channels, ops[j].mod.out_channels) <= 32 and ops[j].mod.weight.requires_grad):
                out.add(i)
    return out


def plan_bn_on_load(prog, ix, training, groups, precision, packed_ids, fused_stats):
    """BatchNorm-on-load: a training-mode BatchNorm(+ReLU) without residual whose ONLY consumer is a 3x3 conv that runs the packed f32x3
    forward and the f32x3 weight gradient is not applied at all - the consumer transforms the BatchNorm's INPUT while staging it
    (kernels.BnOnLoad): one launch and two tensor passes per such layer gone (the inner BatchNorm of every residual unit).  Needs the sums
    from the producer's epilogue (fused_stats) and a table of <= 4 KB.
    packed_ids: id() of the weights the pass's WeightPacker holds, None without a packer."""
    out = set()
    if training and packed_ids is not None and int(precision) in K.SPLIT_PIECES:
        ops = prog.ops
        fused_bn = set(fused_stats.values())
        for i, op in enumerate(ops):
            j = ix.consumer.get(op.dst)
            if (op.kind == "bn" and op.res is None and i in fused_bn and ix.users.get(op.dst, 0) == 1 and j is not None
                    and ops[j].kind == "conv" and ops[j].src == op.dst and ops[j].extra["weight_fn"] is None
                    and not ops[j].extra["in_nchw"] and id(ops[j].mod.weight) in packed_ids
                    and groups * op.mod.num_features * 8 <= 4096):
                out.add(i)
    return out


def plan_joins(prog, ix, training, bn_on_load):
    """join bn op index -> lower bn op index.  Two-branch join: a training-mode BatchNorm whose residual input is itself the output of a
    training-mode BatchNorm that nobody else reads (the lower branch of ResNet50DeconvBlock / the strided ResNet34ConvBlock): the lower
    BatchNorm is not applied on its own - both are applied, added and rectified in ONE pass (kernels.bn_join_fwd), the adjoint is one
    reduce + one apply.  (BatchNorms applied on load by a 3x3 conv are excluded; those of plan_bn_on_load_1x1 are not.)"""
    joins = {}
    if training:
        ops = prog.ops
        for i, op in enumerate(ops):
            j = ix.producer.get(op.res) if (op.kind == "bn" and op.res is not None) else None
            if (j is not None and ops[j].kind == "bn" and ops[j].res is None and not ops[j].relu
                    and ix.users.get(op.res, 0) == 1 and j not in bn_on_load and i not in bn_on_load
                    and op.mod.num_features == ops[j].mod.num_features and op.mod.num_features % 4 == 0
                    and op.mod.weight is not None and ops[j].mod.weight is not None):
                joins[i] = j
    return joins


def plan_bn_pool(prog, ix):
    """BatchNorm (+ReLU) -> MaxPool2d(3, 2, 1), its only consumer: one pass, the activation in between is never stored
    (kernels.bn_maxpool_fwd).  The executor still checks the input's rank and that the batch divides into the statistics groups."""
    ops = prog.ops
    return {i for i, op in enumerate(ops[:-1])
            if op.kind == "bn" and op.res is None and ops[i + 1].kind == "maxpool" and ops[i + 1].src == op.dst
            and op.mod.num_features % 4 == 0 and op.mod.num_features > 1 and ix.users.get(op.dst, 0) == 1}


def plan_folded(prog, ix, fold):
    """bn op index -> conv op index (inference with a fold cache only): every conv whose only consumer is a BatchNorm is deferred to that
    BatchNorm's position and runs with it folded into its weights, the ReLU / residual add fused into its epilogue."""
    folded = {}
    if fold:
        ops = prog.ops
        for i, op in enumerate(ops):
            j = ix.producer.get(op.src)
            if (op.kind == "bn" and j is not None and ops[j].kind == "conv" and ix.users.get(op.src, 0) == 1
                    and not ops[j].extra["out_nchw"] and not ops[j].relu):
                folded[i] = j
    return folded


def plan_forward_arenas(prog, groups, precision):
    """(bn_off, total, nrec).  BatchNorm sums: one zeroed float64 arena for the whole pass (the kernels accumulate with atomics), `bn_off`
    the offset of each BatchNorm's slice.  Precision 4: one zeroed arena of `nrec` magnitude records, one per BatchNorm / transposed-conv
    output (the operands of the fp16-piece 3x3 kernels)."""
    bn_off, total = {}, 0
    for i, op in enumerate(prog.ops):
        if op.kind == "bn":
            bn_off[i] = total
            total += K.bn_stats_doubles(groups, op.mod.num_features)
    nrec = 0
    if int(precision) == K.F16X2:
        nrec = max(1, sum(1 for op in prog.ops if op.kind == "bn" or (op.kind == "conv" and isinstance(op.mod, nn.ConvTranspose2d))))
    return bn_off, total, nrec


def make_forward_plan(prog, training, groups, precision, packed_ids=None, fold=False):
    """The ForwardPlan of one (mode, groups, arithmetic, packer, fold) combination; `precision` as run_forward resolved it."""
    ix = prog.index()
    p = ForwardPlan()
    p.nops = ix.nops
    p.fused_stats = plan_fused_stats(prog, ix, training)
    p.bn_on_load_1x1 = plan_bn_on_load_1x1(prog, ix, training, groups, precision, p.fused_stats)
    p.bn_on_load = plan_bn_on_load(prog, ix, training, groups, precision, packed_ids, p.fused_stats)
    p.consumer = ix.consumer if (training and packed_ids is not None and int(precision) in K.SPLIT_PIECES) else None
    p.joins = plan_joins(prog, ix, training, p.bn_on_load)
    p.join_lower = set(p.joins.values())
    p.bn_pool = plan_bn_pool(prog, ix)
    p.folded = plan_folded(prog, ix, fold)
    p.deferred = set(p.folded.values())
    p.bn_off, p.total, p.nrec = plan_forward_arenas(prog, groups, precision)
    return p


def forward_plan(prog, training, groups, precision, packer, fold):
    """Get-or-make through the program's cache (at most 17 entries: cleared when it outgrows that)."""
    key = forward_key(prog, training, groups, precision, packer, fold)
    p = prog.fw_plans.get(key)
    if p is None:
        if len(prog.fw_plans) > 16:
            prog.fw_plans.clear()
        p = prog.fw_plans[key] = make_forward_plan(prog, training, groups, precision,
                                                   set(packer.entries) if packer is not None else None, fold)
    assert p.nops == len(prog.ops), "Program grew after it first ran"
    prog.last_forward_plan = p
    return p


# -----------------------------------------------------------------------------------------------
# backward
# -----------------------------------------------------------------------------------------------
FROM_1X1_KC = (16,)      # output channels of the 1x1 convs whose dgrad the BatchNorm in front rebuilds (plan_from_1x1)


class BackwardPlan:
    __slots__ = ("nops", "consumed_by", "fuse_bn", "fuse_bias", "from_1x1", "red_off", "bias_off", "total", "nrec")


def backward_key(prog, ctx, gout_shape, want_wgrad):
    """Everything the plan reads that can differ between two backward walks of one program: mode, batch / map geometry via the output
    gradient's shape, the joins made by this forward and the convs it ran - their CONTENTS, not their counts -, the precision, which conv
    weights / biases train (plan_fuse_bias reads the flags: freezing a layer between two steps must not reuse the other plan)."""
    return (bool(ctx.training), bool(want_wgrad), int(ctx.groups), tuple(gout_shape), frozenset(ctx.joined.items()), frozenset(ctx.descs),
            ctx.precision,
            tuple((op.mod.weight.requires_grad, op.mod.bias is not None and op.mod.bias.requires_grad) for op in prog.ops if op.kind == "conv"))


def plan_fuse_bn(prog, ix, ctx):
    """conv op index -> bn op index.  A conv dgrad that COMPLETES the gradient of a training-mode BatchNorm's output (it is the last
    consumer of that slot in backward order) also accumulates that BatchNorm's backward sums in its epilogue (bh_conv_dgrad_bnreduce), so
    the BatchNorm adjoint is one apply launch instead of reduce + finalize + apply."""
    fuse_bn = {}
    if ctx.training:
        ops, descs = prog.ops, ctx.descs
        for j, op in enumerate(ops):
            b = ix.producer.get(op.src)
            if (op.kind == "conv" and b is not None and ops[b].kind == "bn" and ix.last_consumer.get(op.src) == j
                    and j in descs and descs[j].bh_reduce_ok and descs[j].N % ctx.groups == 0 and b not in ctx.joined):
                fuse_bn[j] = b
    return fuse_bn


def plan_fuse_bias(prog, ix, ctx, want_wgrad, fuse_bn):
    """conv op index -> producer op index.  A 3x3 conv that is the ONLY consumer of a biased (transposed) conv's output: the column sums
    of its input gradient are that layer's bias gradient - accumulated in the dgrad epilogue instead of a streaming pass over the
    gradient."""
    fuse_bias = {}
    if want_wgrad:
        ops, descs = prog.ops, ctx.descs
        for j, op in enumerate(ops):
            p = ix.producer.get(op.src)
            if (op.kind == "conv" and j not in fuse_bn and p is not None and ops[p].kind == "conv" and ix.users.get(op.src, 0) == 1
                    and j in descs and p in descs and descs[j].bh_reduce_ok and not ops[p].relu):
                pm = ops[p].mod
                if pm.bias is not None and pm.bias.requires_grad and pm.weight.requires_grad and ops[p].extra["weight_fn"] is None:
                    fuse_bias[j] = p
    return fuse_bias


def plan_from_1x1(prog, ix, ctx, fuse_bn):
    """A 1x1 / stride-1 conv with 16 output channels that is the ONLY consumer of a training-mode BatchNorm (+ReLU, no residual, not
    joined): its dgrad is rebuilt inside that BatchNorm's adjoint (bh_bn_bwd_from_1x1) - the full-resolution decoder unit's 268 MB
    gradient is never written."""
    from_1x1 = set()
    if ctx.training:
        ops = prog.ops
        for j, op in enumerate(ops):
            b = ix.producer.get(op.src)
            m = op.mod
            if (op.kind == "conv" and b is not None and ops[b].kind == "bn" and ops[b].res is None and b not in ctx.joined
                    and ix.users.get(op.src, 0) == 1 and j not in fuse_bn and isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1)
                    and m.stride == (1, 1) and m.padding == (0, 0) and op.extra["weight_fn"] is None and m.out_channels in FROM_1X1_KC
                    and ops[b].mod.num_features % 4 == 0 and 256 % (ops[b].mod.num_features // 4) == 0
                    and not op.extra["in_nchw"] and not op.extra["out_nchw"]):
                from_1x1.add(j)
    return from_1x1


def plan_backward_arenas(prog, ctx, fuse_bn, fuse_bias):
    """(red_off, bias_off, total, nrec): slices of the pass's zeroed float64 arena - the bias column sums first, then the BatchNorm
    backward sums.  Precision 4: `nrec` magnitude records of the BatchNorm input gradients (the gy operand of the fp16-piece dgrad /
    weight-gradient kernels)."""
    red_off, bias_off, total = {}, {}, 0
    for j, p in fuse_bias.items():
        bias_off[p] = total
        total += K.bn_stats_doubles(1, ctx.descs[j].Ci)
    for b in fuse_bn.values():
        red_off[b] = total
        total += K.bn_stats_doubles(ctx.groups, prog.ops[b].mod.num_features)
    nrec = max(1, sum(1 for op in prog.ops if op.kind == "bn")) if ctx.precision == K.F16X2 else 0
    return red_off, bias_off, total, nrec


def make_backward_plan(prog, ctx, want_wgrad):
    """The BackwardPlan for what one forward saved: reads ctx.descs (bh_reduce_ok, N, Ci), .joined, .groups, .training, .precision."""
    ix = prog.index()
    p = BackwardPlan()
    p.nops = ix.nops
    p.consumed_by = ix.users
    p.fuse_bn = plan_fuse_bn(prog, ix, ctx)
    p.fuse_bias = plan_fuse_bias(prog, ix, ctx, want_wgrad, p.fuse_bn)
    p.from_1x1 = plan_from_1x1(prog, ix, ctx, p.fuse_bn)
    p.red_off, p.bias_off, p.total, p.nrec = plan_backward_arenas(prog, ctx, p.fuse_bn, p.fuse_bias)
    return p


def backward_plan(prog, ctx, gout_shape, want_wgrad):
    """Get-or-make through the program's cache (three backward walks per step would otherwise rebuild it)."""
    key = backward_key(prog, ctx, gout_shape, want_wgrad)
    p = prog.bw_plans.get(key)
    if p is None:
        p = prog.bw_plans[key] = make_backward_plan(prog, ctx, want_wgrad)
    assert p.nops == len(prog.ops), "Program grew after it first ran"
    prog.last_backward_plan = p
    return p
