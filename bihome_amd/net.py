"""Conv-stack executor: runs a module tree of Conv2d / ConvTranspose2d / BatchNorm2d / ReLU /
MaxPool2d leaves (the reference's `nn.Module` layout, kept only as the parameter container and
state-dict schema) as a flat program of HIP kernel launches on NHWC feature maps, forward and
backward, without autograd in between.

MI355X-first choices:
  * the reference runs the backbone once per direction (Rethinking.py:296-313) and the extractor once
    per patch (PerceptualHead.py:358-398); here those calls are stacked along the batch axis into ONE
    pass with `groups` independent BatchNorm statistics - half the launches, twice the GEMM M;
  * weights live in [Cout][kh][kw][Cin] order (torch channels_last), which is the K-contiguous B operand
    of the implicit GEMM, so no per-step repacking; gradients are written by the wgrad kernel straight
    into a flat fp32 buffer whose slices are the parameters' `.grad` views (one contiguous RCCL payload);
  * every launch goes to the current HIP stream with static shapes, so a whole step can be captured
    in a HIP graph.

Which launches are fused into their neighbours is decided in plan.py (ForwardPlan / BackwardPlan, cached on the Program);
run_forward / run_backward below execute a plan: one arm per op kind, run-time guards only.
"""
import os
import weakref

import torch
import torch.nn as nn

from . import kernels as K
from . import plan as P


# -----------------------------------------------------------------------------------------------
# parameter layout helpers
# -----------------------------------------------------------------------------------------------
def to_kernel_layout_(module):
    """Re-lay every conv weight in place as channels_last (values and state-dict shapes unchanged)."""
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            if not m.weight.data.is_contiguous(memory_format=torch.channels_last):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return module


def kview(w):
    """[O,I,kh,kw] channels_last parameter -> contiguous [O,kh,kw,I] view (no copy)."""
    if w.dim() == 2:
        return w
    v = w.permute(0, 2, 3, 1)
    if not v.is_contiguous():
        raise RuntimeError("conv weight is not in kernel (channels_last) layout; call net.to_kernel_layout_(module)")
    return v


class FlatGrads:
    """One flat fp32 buffer holding every trainable parameter's gradient; `.grad` of each parameter is a
    view into it laid out like the parameter (so wgrad kernels and the optimizer see the same bytes)."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4          # keep every segment 16 B aligned
        self.numel = n
        self.flat = None
        self.views = None
        self.pflat = None             # round 4: the parameters themselves in a second flat buffer of the same layout (ensure_params)
        self.pviews = None

    def _views_of(self, flat):
        views = []
        for p, off in zip(self.params, self.offsets):
            seg = flat[off:off + p.numel()]
            if p.dim() == 4:
                O, I, kh, kw = p.shape
                v = seg.view(O, kh, kw, I).permute(0, 3, 1, 2)
            else:
                v = seg.view(p.shape)
            views.append(v)
        return views

    def ensure(self, device):
        if self.flat is None or self.flat.device != device:
            self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
            self.views = self._views_of(self.flat)
        return self.flat

    def ensure_params(self, device):
        """The parameters as views into ONE flat buffer laid out like the gradient buffer, so that the optimizer updates one tensor
        instead of ~170 (step.build_optimizer: torch's fused Adam takes 265 us over the tensors of the Zeng backbone and 86 us over the
        same elements in one tensor).  Values are copied once; `p.data` of every parameter becomes its view (state_dict, load_state_dict,
        broadcast and the kernels see the same parameters as before).  Re-run (cheap pointer checks) before every optimizer step: a
        `model.to()`, a re-laid weight or a loader that REPLACES `p.data` is folded back in."""
        if self.pflat is not None and self.pflat.device == device and \
                all(p.data_ptr() == v.data_ptr() for p, v in zip(self.params, self.pviews)):
            return self.pflat
        pflat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        pviews = self._views_of(pflat)
        with torch.no_grad():
            for p, v in zip(self.params, pviews):
                v.copy_(p.data)
                p.data = v
        self.pflat, self.pviews = pflat, pviews
        return pflat

    def attach(self, device):
        """Make sure every parameter's .grad is its view; zero the buffer if any was detached
        (optimizer.zero_grad(set_to_none=True) detaches them all - train.py:305)."""
        self.ensure(device)
        detached = False
        for p, v in zip(self.params, self.views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                detached = True
                break
        if detached:
            self.flat.zero_()
            for p, v in zip(self.params, self.views):
                p.grad = v
        return self.flat


# -----------------------------------------------------------------------------------------------
# program
# -----------------------------------------------------------------------------------------------
class Op:
    __slots__ = ("kind", "src", "dst", "mod", "relu", "res", "extra")

    def __init__(self, kind, src, dst, mod=None, relu=False, res=None, extra=None):
        self.kind, self.src, self.dst, self.mod, self.relu, self.res, self.extra = kind, src, dst, mod, relu, res, extra


class Program:
    """Flat op list over numbered tensor slots. Slot 0 is the input."""

    def __init__(self):
        self.ops = []
        self.nslots = 1
        self._index = None
        self.fw_plans, self.bw_plans = {}, {}             # plan.forward_plan / backward_plan: key -> plan
        self.last_forward_plan = self.last_backward_plan = None

    def index(self):
        """Producer / consumer maps over the op list (plan.ProgramIndex), made once: a program is built in one go and not extended after
        it first ran (the plans made from a shorter op list are dropped if it is)."""
        if self._index is None or self._index.nops != len(self.ops):
            self.fw_plans.clear()
            self.bw_plans.clear()
            self._index = P.ProgramIndex(self.ops)
        return self._index

    def plans(self):
        """The fusion plans kept on this program and the two that the most recent forward / backward pass ran with."""
        return {"forward": dict(self.fw_plans), "backward": dict(self.bw_plans),
                "last_forward": self.last_forward_plan, "last_backward": self.last_backward_plan}

    def invalidate(self):
        """Drop everything derived from the op list and the conv geometry: the index, the plans and the memoised descriptors."""
        self._index = None
        self.fw_plans.clear()
        self.bw_plans.clear()
        self.last_forward_plan = self.last_backward_plan = None
        _GEOM_CACHE.clear()

    def _new(self):
        self.nslots += 1
        return self.nslots - 1

    def conv(self, src, mod, in_nchw=False, out_nchw=False, weight_fn=None, relu=False):
        """relu: the activation in the conv's own epilogue (bh_conv_fwd_act) - a conv / Linear followed directly by nn.ReLU, no BatchNorm
        in between (the projection head's layers); its adjoint masks the output gradient first (kernels.relu_bwd)."""
        dst = self._new()
        self.ops.append(Op("conv", src, dst, mod, relu=relu, extra={"in_nchw": in_nchw, "out_nchw": out_nchw, "weight_fn": weight_fn}))
        return dst

    def bn(self, src, mod, relu=False, res=None):
        dst = self._new()
        self.ops.append(Op("bn", src, dst, mod, relu=relu, res=res))
        return dst

    def tail(self, src, conv1, bn, conv2):
        """Fused Conv1x1 + BatchNorm + ReLU + Conv1x1 -> NCHW (bh_tail_fwd/bwd)."""
        dst = self._new()
        self.ops.append(Op("tail", src, dst, (conv1, bn, conv2)))
        return dst

    def maxpool(self, src):
        dst = self._new()
        self.ops.append(Op("maxpool", src, dst))
        return dst

    def gap(self, src):
        dst = self._new()
        self.ops.append(Op("gap", src, dst))
        return dst

    # ---- builders for the reference's block types -------------------------------------------
    def sequential(self, src, seq):
        """nn.Sequential of Conv/ConvT/BN/ReLU/MaxPool leaves and residual blocks (in reference order)."""
        mods = list(seq)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                src = self.conv(src, m, relu=relu)
                if relu:
                    i += 1
            elif isinstance(m, nn.BatchNorm2d):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                src = self.bn(src, m, relu=relu)
                if relu:
                    i += 1
            elif isinstance(m, nn.MaxPool2d):
                src = self.maxpool(src)
            elif hasattr(m, "upper_branch"):
                src = self.residual(src, m)
            else:
                raise TypeError("unsupported leaf %r" % type(m))
            i += 1
        return src

    def residual(self, src, blk):
        """ReLU(upper_branch(x) + lower_branch(x) | x)  (src/backbones/utils.py:60-131): the last BN of the
        upper branch takes the lower result as fused residual input and applies the ReLU."""
        low = src
        if getattr(blk, "lower_branch", None) is not None and len(list(blk.lower_branch)) > 0:
            low = self.sequential(src, blk.lower_branch)
        up = list(blk.upper_branch)
        assert isinstance(up[-1], nn.BatchNorm2d)
        mid = self.sequential(src, up[:-1])
        return self.bn(mid, up[-1], relu=True, res=low)

    def basic_block(self, src, blk):
        """torchvision BasicBlock(conv1,bn1,relu,conv2,bn2,downsample)."""
        low = src
        if blk.downsample is not None:
            low = self.sequential(src, blk.downsample)
        t = self.bn(self.conv(src, blk.conv1), blk.bn1, relu=True)
        return self.bn(self.conv(t, blk.conv2), blk.bn2, relu=True, res=low)


class Ctx:
    """Saved tensors of one forward pass."""
    __slots__ = ("slots", "stats", "descs", "groups", "training", "weights", "wkeys", "wpacked", "precision", "joined")

    def __init__(self):
        self.slots, self.stats, self.descs, self.weights, self.wkeys, self.wpacked = {}, {}, {}, {}, {}, {}
        self.joined = {}          # join BatchNorm op index -> lower-branch BatchNorm op index (kernels.bn_join_fwd)
        self.precision = 0


_GEOM_CACHE = {}
X3_WS_BYTES = 40 << 20          # Runner.x3_workspace: partial blocks of the f32x3 weight gradient
DET_WS_BYTES = 256 << 20        # deterministic mode: partial tiles / integer-limb shadow entries of ANY layer's weight gradient
                                # (32 bytes per weight: 75.5 MB for a 512 x 512 x 3 x 3 layer)


def _conv_geometry(mod, x_shape, in_nchw, out_nchw, precision=0):
    """Conv descriptor for `mod` on an input of `x_shape`, memoised together with what the library reports for it (halo
    3x3 kernel eligible for packed weights / for the fused BatchNorm reduce) and its packed-layout twin: building the
    ctypes struct and asking bh_conv_variant costs ~20 us of host time per launch otherwise, which is what bounds the
    shorter models (ResNet-34 regressor: 13.1 -> 15-17 ms/step when it was done per call)."""
    key = (id(mod), tuple(x_shape), bool(in_nchw), bool(out_nchw), int(precision), K.deterministic())   # (the workspace bytes depend on the mode)
    hit = _GEOM_CACHE.get(key)
    if hit is not None and hit[0] is mod:
        return hit[1]
    d = _conv_geometry_uncached(mod, x_shape, in_nchw, out_nchw, precision)
    d.bh_packs = bool(isinstance(mod, nn.Conv2d) and K.packs_3x3(d))
    d.bh_reduce_ok = bool(isinstance(mod, nn.Conv2d) and K.dgrad_bn_reduce_ok(d))
    d.bh_packed = K._with_layout(d, K.packed_layout(precision)) if d.bh_packs else None
    # f32x3 weight gradient (csrc/wgrad_x3.hip): reduces its split-K partial blocks through a workspace (fixed order, cheaper than atomics)
    d.bh_wx3 = bool(int(precision) in K.SPLIT_PIECES and isinstance(mod, nn.Conv2d) and K.conv_variant(d, "wgrad").startswith("wgrad_x3"))
    d.bh_wx3_bytes = K.wgrad_det_bytes(d) if d.bh_wx3 else 0
    _GEOM_CACHE[key] = (mod, d)
    return d


def _conv_geometry_uncached(mod, x_shape, in_nchw, out_nchw, precision=0):
    if in_nchw:
        N, Ci, Hi, Wi = x_shape
    else:
        N, Hi, Wi, Ci = x_shape
    if isinstance(mod, nn.Linear):
        return K.conv_desc(N, Hi, Wi, Ci, mod.out_features, 1, 1, 0, precision=precision)
    k, s, p = mod.kernel_size[0], mod.stride[0], mod.padding[0]
    tr = isinstance(mod, nn.ConvTranspose2d)
    Co = mod.out_channels
    return K.conv_desc(N, Hi, Wi, Ci, Co, k, s, p, transposed=tr, in_nchw=in_nchw, out_nchw=out_nchw, precision=precision)


def _folded(cache, conv, bn, weight_fn):
    """Eval-mode BatchNorm folded into the preceding conv: w' = w * s[co], b' = b * s + t with s = gamma / sqrt(var + eps),
    t = beta - mean * s (running statistics).  Cached per (conv, bn) pair until a parameter / buffer version changes."""
    key = (id(conv), id(bn))
    vers = tuple(t._version for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
                 if t is not None)
    hit = cache.get(key)
    if hit is not None and hit[0] == vers:
        return hit[1], hit[2]
    with torch.no_grad():
        s = torch.rsqrt(bn.running_var + bn.eps)
        if bn.weight is not None:
            s = s * bn.weight
        t = -bn.running_mean * s
        if bn.bias is not None:
            t = t + bn.bias
        w = weight_fn(conv.weight) if weight_fn else conv.weight
        if isinstance(conv, nn.ConvTranspose2d):                  # [Ci, Co, kh, kw]
            wf = (w * s.view(1, -1, 1, 1)).contiguous(memory_format=torch.channels_last)
        elif w.dim() == 4:
            wf = (w * s.view(-1, 1, 1, 1)).contiguous(memory_format=torch.channels_last)
        else:
            wf = (w * s.view(-1, 1)).contiguous()
        bf = (conv.bias * s + t) if conv.bias is not None else t
        bf = bf.contiguous()
    cache[key] = (vers, wf, bf)
    return wf, bf


def _momentum(bn):
    """torch's momentum=None (cumulative moving average) is not built: the kernels replay one exponential update per
    statistics group.  No reference module uses it (every BatchNorm2d upstream keeps the default 0.1)."""
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not supported by bihome_amd")
    return bn.momentum


def _zero_arenas(n_doubles, n_floats, device):
    """The two zeroed scratch arenas of a pass - float64 sums and float32 magnitude records - out of ONE zero-filled byte buffer (one fill
    launch instead of two, five times per training step).  Either may be empty (None)."""
    if not (n_doubles or n_floats):
        return None, None
    buf = torch.zeros(n_doubles * 8 + n_floats * 4, dtype=torch.uint8, device=device)
    a = buf[:n_doubles * 8].view(torch.float64) if n_doubles else None
    b = buf[n_doubles * 8:].view(torch.float32) if n_floats else None
    return a, b


class _FwPass:
    """What the arms of one run_forward call share (one object per pass)."""
    __slots__ = ("prog", "plan", "slots", "ready", "arena", "amax_next", "ctx", "save", "groups", "training", "precision", "packer",
                 "fold_cache", "input_source")


def _bn_stats_slice(s, i, C):
    """The float64 sums of BatchNorm op `i` (C channels) in the pass's zeroed arena."""
    off = s.plan.bn_off[i]
    return s.arena[off:off + K.bn_stats_doubles(s.groups, C)]


def _count_batch(m, groups):
    """Flushed to the `num_batches_tracked` buffer lazily (flush_counters): no per-layer launch."""
    m._bh_pending_batches = getattr(m, "_bh_pending_batches", 0) + groups


def _fw_folded_conv(s, i, op):
    """Inference: the conv deferred to its BatchNorm's position `i`, with the BatchNorm folded into its weights."""
    cop = s.prog.ops[s.plan.folded[i]]
    e, slots, fold_cache, precision = cop.extra, s.slots, s.fold_cache, s.precision
    csrc = slots[cop.src]
    d = _conv_geometry(cop.mod, csrc.shape, e["in_nchw"], e["out_nchw"], precision)
    wf, bf = _folded(fold_cache, cop.mod, op.mod, e["weight_fn"])
    pf = None
    if precision in K.SPLIT_PIECES and d.bh_packs and e["weight_fn"] is None:
        # f32x3 inference: the folded weights in cut fragment order (packed once per fold)
        ent = fold_cache[(id(cop.mod), id(op.mod))]
        if len(ent) < 4 or ent[3] is None:
            pk = K.packer_for_precision(precision)
            pf, _ = pk.get(wf, need_dgrad=False)
            pk.refresh()
            fold_cache[(id(cop.mod), id(op.mod))] = (ent[0], ent[1], ent[2], pf)
        else:
            pf = ent[3]
    return K.conv_fwd(csrc, kview(wf), bf, d, res=slots[op.res] if op.res is not None else None, relu=op.relu, wpacked=pf,
                      warp_src=s.input_source if cop.src == 0 else None)


def _fw_conv(s, i, op, src):
    e, packer, groups, amax_next = op.extra, s.packer, s.groups, s.amax_next
    d = _conv_geometry(op.mod, src.shape, e["in_nchw"], e["out_nchw"], s.precision)
    w = e["weight_fn"](op.mod.weight) if e["weight_fn"] else op.mod.weight
    wk = kview(w)
    pk = None
    if packer is not None and e["weight_fn"] is None and d.bh_packs and id(op.mod.weight) in packer.entries:
        pk = packer.entries[id(op.mod.weight)]
    wsrc = s.input_source if op.src == 0 else None
    fused_stats = s.plan.fused_stats
    if op.relu:
        out = K.conv_fwd(src, wk, op.mod.bias, d, relu=True, wpacked=pk[1] if pk else None, warp_src=wsrc)
    elif i in fused_stats and d.N % groups == 0:
        b = fused_stats[i]
        out = K.conv_fwd(src, wk, op.mod.bias, d, bn_sums=_bn_stats_slice(s, b, d.Co), groups=groups,
                         wpacked=pk[1] if pk else None, warp_src=wsrc)
        s.ready.add(b)
    elif amax_next and pk is None and isinstance(op.mod, nn.ConvTranspose2d) and not e["out_nchw"]:
        # a transposed conv in front of a packed fp16-piece 3x3 conv (the decoder units): the magnitude record of its output from
        # its own epilogue instead of a bh_absmax pass over the (up to 268 MB) tensor
        out = K.conv_fwd(src, wk, op.mod.bias, d, amax=amax_next(), warp_src=wsrc)
    else:
        out = K.conv_fwd(src, wk, op.mod.bias, d, wpacked=pk[1] if pk else None, warp_src=wsrc)
    if s.save:
        ctx = s.ctx
        ctx.descs[i], ctx.weights[i] = d, wk
        ctx.wpacked[i] = pk[2] if pk else None
        ctx.wkeys[i] = (op.mod.weight, op.mod.weight._version)
    return out


def _bn_on_load_ok(s, i, op, src):
    """Run-time half of the BatchNorm-on-load decisions (plan.plan_bn_on_load / plan_bn_on_load_1x1): the sums came from the producer's
    epilogue, the batch divides into the statistics groups, and the consumer can take the un-materialised operand."""
    m, groups, plan = op.mod, s.groups, s.plan
    if i in plan.bn_on_load_1x1 and i in s.ready and src.shape[0] % groups == 0 and (src.numel() // (m.num_features * groups)) % 128 == 0:
        return True
    if i in plan.bn_on_load and i in s.ready and src.shape[0] % groups == 0:
        cop = s.prog.ops[plan.consumer[op.dst]]
        cd = _conv_geometry(cop.mod, src.shape, False, cop.extra["out_nchw"], s.precision)
        # (the consumer's weight gradient must fit the fixed f32x3 workspace, else its backward could not take the
        #  un-materialised operand: decided here, before the BatchNorm output is elided)
        return bool(cd.bh_packs and cd.bh_wx3 and 0 < cd.bh_wx3_bytes <= (DET_WS_BYTES if K.deterministic() else X3_WS_BYTES))
    return False


def _fw_bn(s, i, op, src):
    m, plan, groups, training, amax_next = op.mod, s.plan, s.groups, s.training, s.amax_next
    res = s.slots[op.res] if op.res is not None else None
    if i in plan.join_lower and src.shape[0] % groups == 0:
        # the lower branch of a join: statistics only (from the producer's epilogue, else one pass); applied inside the join
        st = _bn_stats_slice(s, i, m.num_features)
        if i not in s.ready:
            K.bn_stats(src, st, groups, m.num_features)
        out = K.BnJoinPending(src, st, m)
    elif i in plan.joins and isinstance(res, K.BnJoinPending) and src.shape[0] % groups == 0:
        st = _bn_stats_slice(s, i, m.num_features)
        if i not in s.ready:
            K.bn_stats(src, st, groups, m.num_features)
        out = K.bn_join_fwd(src, res.x, m, res.mod, st, res.stats, groups, op.relu, _momentum(m), _momentum(res.mod),
                            amax=amax_next() if amax_next else None)
        if s.save:
            s.ctx.joined[i] = plan.joins[i]
    else:
        if isinstance(res, K.BnJoinPending):          # (a join that could not be formed after all: apply the lower BatchNorm now)
            lo, _ = K.bn_fwd(res.x, res.mod.weight, res.mod.bias, res.mod.running_mean, res.mod.running_var, None, groups, res.mod.eps,
                             _momentum(res.mod), False, training, stats=res.stats, stats_ready=True)
            res = s.slots[op.res] = lo
        st = _bn_stats_slice(s, i, m.num_features)
        if i in plan.bn_pool and src.dim() == 4 and src.shape[0] % groups == 0:
            out = K.bn_maxpool_fwd(src, m.weight, m.bias, m.running_mean, m.running_var, groups, m.eps, _momentum(m), op.relu,
                                   training, st, i in s.ready, want_index=s.save, amax=amax_next() if amax_next else None)
        elif _bn_on_load_ok(s, i, op, src):
            rec = amax_next() if amax_next else None
            table = K.bn_fwd_coeffs(st, m.weight, m.bias, m.running_mean, m.running_var, groups,
                                    src.numel() // (m.num_features * groups), m.num_features, m.eps, _momentum(m), amax=rec)
            out = K.BnOnLoad(src, table, groups, op.relu, amax=rec)
        else:
            out, st = K.bn_fwd(src, m.weight, m.bias, m.running_mean, m.running_var, res, groups, m.eps, _momentum(m), op.relu, training,
                               stats=st, stats_ready=i in s.ready, amax=amax_next() if (amax_next and m.num_features > 1) else None)
    if training:            # (joins are planned in training mode only)
        _count_batch(m, groups)
    if s.save:
        s.ctx.stats[i] = st
    return out


def _fw_tail(s, i, op, src):
    c1, bn, c2 = op.mod
    N, h, w, _ = src.shape
    out, ws = K.tail_fwd(src, kview(c1.weight), c1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                         kview(c2.weight), c2.bias, s.groups, h * w, bn.eps, _momentum(bn), s.training)
    if s.training:
        _count_batch(bn, s.groups)
    if s.save:
        s.ctx.stats[i] = ws
    return out


def _fw_maxpool(s, i, op, src):
    if isinstance(src, K.BnPooled):               # pooled by the fused BatchNorm kernel already
        out, idx = src.pooled, src.idx
    else:
        out, idx = K.maxpool_fwd(src, want_index=s.save)
    if s.save:
        s.ctx.stats[i] = idx
    return out


def _fw_gap(s, i, op, src):
    return K.gap_fwd(src)


_FW_ARMS = {"conv": _fw_conv, "bn": _fw_bn, "tail": _fw_tail, "maxpool": _fw_maxpool, "gap": _fw_gap}


def run_forward(prog, x, groups, training, save, precision=0, fold_cache=None, packer=None, input_source=None):
    """packer: kernels.WeightPacker holding fragment-ordered copies of the 3x3 weights (refreshed here, one launch, when
    a parameter changed): the halo-tiled 3x3 kernel then streams its B operand straight into registers.
    x: NHWC (or NCHW when the first conv is flagged in_nchw). Returns (out, ctx|None).
    fold_cache (inference only: not training, nothing saved): a dict - every conv whose only consumer is a BatchNorm
    runs with that BatchNorm folded into its weights and the ReLU / residual add fused into its epilogue.
    input_source: x is an unfilled buffer - the homography warp of input_source["src"], which the conv that reads the input
    makes on the way (kernels.conv_fwd warp_src) or has made in front of it."""
    precision = int(precision)
    if precision == K.F16X2 and (packer is None or not packer.f16):
        # the fp16-piece kernels exist for packed weights with magnitude records of their operands (the BatchNorm kernels of a
        # training-style pass leave them); the BatchNorm-folded inference pass runs the exact three-piece arithmetic
        precision = 2
    if packer is not None:
        # a forward that saves for backward is (probably) followed by an optimizer step, whatever module.training says
        # (frozen-BatchNorm fine-tuning runs the backbone in eval() mode): fused optimizers do not bump version counters
        packer.refresh(training or save)
    plan = P.forward_plan(prog, training, groups, precision, packer, fold_cache is not None and not training and not save)
    s = _FwPass()
    s.prog, s.plan, s.groups, s.training, s.save, s.precision = prog, plan, groups, training, save, precision
    s.packer, s.fold_cache, s.input_source = packer, fold_cache, input_source
    s.slots = slots = {0: x}
    s.ready = set()
    s.ctx = ctx = Ctx() if save else None
    if save:
        ctx.groups, ctx.training, ctx.precision = groups, training, precision
    s.arena, amax_arena = _zero_arenas(plan.total, plan.nrec * K.AMAX_FLOATS, x.device)          # (one fill launch for both)
    s.amax_next = iter(amax_arena.split(K.AMAX_FLOATS)).__next__ if plan.nrec else None
    folded, deferred, arms = plan.folded, plan.deferred, _FW_ARMS
    for i, op in enumerate(prog.ops):
        if i in deferred:
            continue
        if i in folded:
            slots[op.dst] = _fw_folded_conv(s, i, op)
        else:
            slots[op.dst] = arms[op.kind](s, i, op, slots.get(op.src))
    if save:
        ctx.slots = slots
    return slots[prog.ops[-1].dst], ctx


_SIDE_STREAMS = {}


def side_stream(device):
    """The per-device HIP stream that carries the weight-gradient GEMMs (and the head's feature prefetch): they have no
    consumer inside the backward chain, so they run under the dgrad / BatchNorm kernels of the main stream."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return _SIDE_STREAMS[key]


class _BwPass:
    """What the arms of one run_backward call share (one object per pass)."""
    __slots__ = ("prog", "plan", "ctx", "slots", "grads", "bn_reduced", "red_arena", "amax_next", "want_wgrad", "want_input_grad",
                 "on_param_grad", "wgrad_stream", "main", "det_ws", "x3_ws", "input_sink")


def _contribute(grads, slot, g):
    if slot in grads:
        K.add_(grads[slot], g)
    else:
        grads[slot] = g


def _params_ready(s, *params):
    """The gradients of these parameters are final: their bucket may leave."""
    if s.on_param_grad is not None:
        for p in params:
            if p is not None:
                s.on_param_grad(p)


def _enqueue_wgrad(s, i, op, g, x, d):
    """Weight (and bias) gradient of conv op `i`: on the side stream behind an event when there is one (g is final here)."""
    m, wgrad_stream, red_arena, bias_off = op.mod, s.wgrad_stream, s.red_arena, s.plan.bias_off
    gw = m.weight.grad if m.weight.dim() == 2 else kview(m.weight.grad)
    gb = m.bias.grad if (m.bias is not None and m.bias.requires_grad) else None
    has_gb = gb is not None
    if i in bias_off and has_gb:              # column sums already taken by the consumer's dgrad epilogue
        K.bias_grad_from_sums(red_arena[bias_off[i]:bias_off[i] + K.bn_stats_doubles(1, d.Co)], gb, 1, d.Co)
        gb = None
    ws = s.det_ws if s.det_ws is not None else (s.x3_ws if d.bh_wx3 else None)
    # the fp16-piece weight gradient's eight-wave form is the faster launch alone, the four-wave form the better neighbour: it
    # leaves ~200 registers per SIMD lane, so the main stream's BatchNorm kernels run ON the same CUs (same-box A/B:
    # two streams 13.30 ms with the four-wave form against 13.49; one stream 14.13 against 14.02)
    # and with 160 instead of 256 workgroups the side stream leaves CUs to the main stream's next launch (and writes fewer partial
    # blocks): two streams 12.60 against 12.79 ms (ROUTE_WX3_SHARED)
    if wgrad_stream is None:
        d.route = (d.route | K.ROUTE_WX3_PC) & ~K.ROUTE_WX3_SHARED
    else:
        d.route = (d.route & ~K.ROUTE_WX3_PC) | K.ROUTE_WX3_SHARED
    if wgrad_stream is None:
        K.conv_wgrad(x, g, gw, gb, d, det_ws=ws)
    else:
        if s.ctx.precision == K.F16X2 and d.bh_wx3:
            # magnitude records the fp16-piece weight gradient reads: made (if missing) on the MAIN stream, in front of the
            # event - a record first measured on the side stream would be read by the main stream's dgrad without a wait
            # (a still-zero record scales by 2^127)
            K.amax_of(g)
            K.amax_of(x)
        ev = torch.cuda.Event()
        ev.record(s.main)                                 # g is final here
        g.record_stream(wgrad_stream)
        with torch.cuda.stream(wgrad_stream):
            wgrad_stream.wait_event(ev)
            K.conv_wgrad(x, g, gw, gb, d, det_ws=ws if d.bh_wx3 else None)     # (one stream: launches serialise on the workspace)
    _params_ready(s, m.weight, m.bias if has_gb else None)


def _bw_conv(s, i, op, g, x, need_src_grad):
    ctx, plan, grads = s.ctx, s.plan, s.grads
    d, wk = ctx.descs[i], ctx.weights[i]
    if op.relu:                                   # the activation ran in this conv's epilogue: its adjoint in front of everything else
        g = K.relu_bwd(g, s.slots[op.dst])
    if s.want_wgrad and op.mod.weight.requires_grad and op.extra["weight_fn"] is None:
        _enqueue_wgrad(s, i, op, g, x, d)
    if not need_src_grad:
        return
    if i in plan.from_1x1 and op.src not in grads:
        # the BatchNorm in front rebuilds this dgrad per element in its own adjoint (bn_bwd_from_1x1): nothing is launched here
        grads[op.src] = K.GradFrom1x1(g, wk)
        return
    red = None
    if i in plan.fuse_bn:
        b = plan.fuse_bn[i]
        bop, bm = s.prog.ops[b], s.prog.ops[b].mod
        sums = s.red_arena[plan.red_off[b]:plan.red_off[b] + K.bn_stats_doubles(ctx.groups, bm.num_features)]
        red = dict(z=s.slots[bop.src], y=s.slots[bop.dst] if (bop.relu and bop.res is not None) else None,
                   stats=ctx.stats[b], gamma=bm.weight, beta=bm.bias, eps=bm.eps, relu=bop.relu, sums=sums,
                   groups=ctx.groups)
        s.bn_reduced[b] = sums
    if i in plan.fuse_bias and op.src not in grads and red is None:
        p = plan.fuse_bias[i]
        grads[op.src] = K.conv_dgrad(g, wk, d, wpacked=ctx.wpacked.get(i),
                                     colsum=s.red_arena[plan.bias_off[p]:plan.bias_off[p] + K.bn_stats_doubles(1, d.Ci)])
    elif op.src in grads:
        K.conv_dgrad(g, wk, d, out=grads[op.src], bn_reduce=red, wkey=ctx.wkeys[i], wpacked=ctx.wpacked.get(i))
    else:
        # (input_sink: the consumer of the INPUT's gradient folded into the first conv's dgrad - the warp's adjoint)
        gsrc = K.conv_dgrad(g, wk, d, bn_reduce=red, wkey=ctx.wkeys[i], wpacked=ctx.wpacked.get(i),
                            warp_sink=s.input_sink if (op.src == 0 and red is None) else None)
        if gsrc is not None:
            grads[op.src] = gsrc


def _bw_bn_join(s, i, op, g, x, need_src_grad):
    ctx, slots, amax_next = s.ctx, s.slots, s.amax_next
    j = ctx.joined[i]
    lop, m, lm = s.prog.ops[j], op.mod, s.prog.ops[j].mod
    train_a = s.want_wgrad and m.weight.requires_grad
    train_b = s.want_wgrad and lm.weight.requires_grad
    xb = slots[lop.src]
    gxa, gxb = K.bn_join_bwd(g, slots[op.dst], x, xb, m, lm, ctx.stats[i], ctx.stats[j], ctx.groups, op.relu, train_a, train_b,
                             amax_a=amax_next() if amax_next else None, amax_b=amax_next() if amax_next else None)
    if train_a:
        _params_ready(s, m.weight, m.bias)
    if train_b:
        _params_ready(s, lm.weight, lm.bias)
    if need_src_grad:
        _contribute(s.grads, op.src, gxa)
    if (lop.src != 0) or s.want_input_grad:
        _contribute(s.grads, lop.src, gxb)


def _bw_bn(s, i, op, g, x, need_src_grad):
    m, ctx, amax_next = op.mod, s.ctx, s.amax_next
    train_w = s.want_wgrad and m.weight is not None and m.weight.requires_grad
    ggamma, gbeta = (m.weight.grad, m.bias.grad) if train_w else (None, None)
    amax = amax_next() if (amax_next and m.num_features > 1) else None
    gres = None
    if isinstance(g, K.GradFrom1x1):             # the 1x1 conv behind this BatchNorm left its dgrad to this call
        gx = K.bn_bwd_from_1x1(g, x, m.weight, m.bias, ctx.stats[i], ctx.groups, m.eps, op.relu, ggamma, gbeta, amax=amax)
    elif isinstance(g, K.PooledGrad):            # BatchNorm (+ReLU) + MaxPool in one pass: its adjoint in one call too
        gx = K.bn_maxpool_bwd(g, x, m.weight, m.bias, ctx.stats[i], m.running_mean, m.running_var, ctx.groups, m.eps, op.relu,
                              ctx.training, ggamma, gbeta, amax=amax)
    else:
        yb = s.slots[op.dst]
        if isinstance(yb, (K.BnOnLoad, K.BnPooled)):  # applied on load by its consumer / fused with the pooling: no output tensor (the mask comes from x)
            yb = None
        gx, gres = K.bn_bwd(g, yb, x, m.weight, ctx.stats[i], m.running_mean, m.running_var, ctx.groups,
                            m.eps, op.relu, ctx.training, op.res is not None and ((op.res != 0) or s.want_input_grad),
                            ggamma, gbeta, beta=m.bias, had_res=op.res is not None, sums_ready=s.bn_reduced.get(i), amax=amax)
    if train_w and s.on_param_grad is not None:
        s.on_param_grad(m.weight)
        s.on_param_grad(m.bias)
    if need_src_grad:
        _contribute(s.grads, op.src, gx)
    if gres is not None:
        _contribute(s.grads, op.res, gres)


def _bw_tail(s, i, op, g, x, need_src_grad):
    ctx = s.ctx
    c1, bn, c2 = op.mod
    tr = s.want_wgrad and c1.weight.requires_grad
    N, h, w, _ = x.shape
    eval_b1 = tr and not ctx.training and c1.bias is not None and c1.bias.requires_grad
    gbeta0 = bn.bias.grad.clone() if eval_b1 else None
    gx = K.tail_bwd(g, x, kview(c1.weight), c1.bias, bn.weight, bn.bias, kview(c2.weight), ctx.stats[i],
                    bn.running_mean, bn.running_var, ctx.groups, h * w, bn.eps, ctx.training, need_src_grad,
                    kview(c1.weight.grad) if tr else None, bn.weight.grad if tr else None,
                    bn.bias.grad if tr else None, kview(c2.weight.grad) if tr else None,
                    c2.bias.grad if (tr and c2.bias is not None) else None)
    if eval_b1:
        # eval-mode BatchNorm is a fixed affine map, so layer8.0.bias has a gradient (with batch statistics it is
        # exactly zero and the fused kernel never forms it): g_b1 = g_beta * gamma / sqrt(running_var + eps)
        with torch.no_grad():
            c1.bias.grad.add_((bn.bias.grad - gbeta0) * bn.weight * torch.rsqrt(bn.running_var + bn.eps))
    if tr:
        _params_ready(s, c2.weight, c2.bias, bn.weight, bn.bias, c1.weight, c1.bias)
    if need_src_grad:
        _contribute(s.grads, op.src, gx)


def _bw_maxpool(s, i, op, g, x, need_src_grad):
    if need_src_grad:
        if isinstance(x, K.BnPooled) and op.src not in s.grads:
            s.grads[op.src] = K.PooledGrad(g, s.ctx.stats[i])          # (consumed by the BatchNorm's adjoint: bn_maxpool_bwd)
        else:
            _contribute(s.grads, op.src, K.maxpool_bwd(s.ctx.stats[i], g, tuple(x.shape)))


def _bw_gap(s, i, op, g, x, need_src_grad):
    if need_src_grad:
        _contribute(s.grads, op.src, K.gap_bwd(g, tuple(x.shape)))


_BW_ARMS = {"conv": _bw_conv, "bn": _bw_bn, "tail": _bw_tail, "maxpool": _bw_maxpool, "gap": _bw_gap}


def run_backward(prog, ctx, gout, want_wgrad, want_input_grad, on_param_grad=None, wgrad_stream=None, det_ws=None, x3_ws=None, input_sink=None):
    """Adjoint of run_forward. Parameter gradients are accumulated (+=) into each parameter's `.grad`
    tensor (which must already exist, see FlatGrads). Returns the input gradient or None.
    wgrad_stream: a second HIP stream for the conv weight-gradient launches.  The backward chain on the main stream is
    dgrad -> BatchNorm backward -> dgrad ...: the wgrad of a layer only needs that layer's output gradient, so it is
    enqueued behind an event and overlaps the chain (MFMA-bound wgrad under the HBM-bound BatchNorm kernels); the
    main stream joins the side stream before returning."""
    main = torch.cuda.current_stream() if wgrad_stream is not None else None
    if wgrad_stream is not None:
        wgrad_stream.wait_stream(main)          # activations, zeroed gradient buffer
    plan = P.backward_plan(prog, ctx, gout.shape, want_wgrad)
    s = _BwPass()
    s.prog, s.plan, s.ctx, s.slots, s.main, s.wgrad_stream = prog, plan, ctx, ctx.slots, main, wgrad_stream
    s.want_wgrad, s.want_input_grad, s.on_param_grad = want_wgrad, want_input_grad, on_param_grad
    s.det_ws, s.x3_ws, s.input_sink = det_ws, x3_ws, input_sink
    s.grads = grads = {prog.ops[-1].dst: gout}
    s.bn_reduced = {}
    s.red_arena, amax_arena = _zero_arenas(plan.total, plan.nrec * K.AMAX_FLOATS, gout.device)    # (one fill launch for both)
    s.amax_next = iter(amax_arena.split(K.AMAX_FLOATS)).__next__ if plan.nrec else None
    ops, slots, joined, arms = prog.ops, ctx.slots, ctx.joined, _BW_ARMS
    for i in range(len(ops) - 1, -1, -1):
        op = ops[i]
        g = grads.pop(op.dst, None)
        if g is None:
            continue
        arm = _bw_bn_join if (op.kind == "bn" and i in joined) else arms[op.kind]
        arm(s, i, op, g, slots[op.src], (op.src != 0) or want_input_grad)
    if wgrad_stream is not None:
        main.wait_stream(wgrad_stream)          # the optimiser (and the release of the activations) follows
    return grads.get(0)


def _drop_pending_counters(module, *unused):
    for m in module.modules():
        if getattr(m, "_bh_pending_batches", 0):
            m._bh_pending_batches = 0


def install_counter_hooks(module):
    """load_state_dict replaces `num_batches_tracked`: calls counted on the host before the load must not be added on
    top of the loaded value at the next state_dict()."""
    module.register_load_state_dict_pre_hook(lambda *a, **k: _drop_pending_counters(module))
    return module


def flush_counters(module):
    """Write the BatchNorm call counters accumulated on the host into the `num_batches_tracked`
    buffers (kept for state-dict compatibility with the reference's checkpoints)."""
    for m in module.modules():
        n = getattr(m, "_bh_pending_batches", 0)
        if n and getattr(m, "num_batches_tracked", None) is not None:
            m.num_batches_tracked += n
            m._bh_pending_batches = 0


class NetFunction(torch.autograd.Function):
    """One autograd node for a whole conv stack: forward = run_forward, backward = run_backward.
    `anchor` is any trainable parameter of the stack (or a dummy): it only tells autograd that the
    node has trainable state; parameter gradients are written by the kernels into `.grad` directly."""

    @staticmethod
    def forward(ctx, x, anchor, runner, groups, grad_mode=True):
        with K.det_scope(runner.det):               # every launch of this pass carries the Runner's own determinism bit
            return NetFunction._forward(ctx, x, anchor, runner, groups, grad_mode)

    @staticmethod
    def backward(ctx, g):
        with K.det_scope(ctx.runner.det):
            return NetFunction._backward(ctx, g)

    @staticmethod
    def _forward(ctx, x, anchor, runner, groups, grad_mode=True):
        # (needs_input_grad reflects requires_grad of the inputs even under torch.no_grad(): the caller passes the mode)
        need = grad_mode and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        training = runner.module.training
        if training or need:
            # running statistics (training) or the weights (a backward + fused optimizer step follows: no version bump) are
            # about to change under the folded copies
            runner._fold.clear()
        fold = runner._fold if (runner.fold_bn and not training and not need) else None
        source = getattr(runner, "input_source", None)
        out, saved = run_forward(runner.prog, x, groups, training, save=need, precision=runner.precision, fold_cache=fold,
                                 packer=runner.packer_for(x.device) if fold is None else None, input_source=source)
        if source is not None and not source.get("filled"):
            raise RuntimeError("input_source: no conv reads the network's input directly - nobody made the warped image")
        ctx.runner, ctx.saved, ctx.want_x = runner, saved, ctx.needs_input_grad[0]
        return out

    @staticmethod
    def _backward(ctx, g):
        r = ctx.runner
        if r.flat is not None:
            r.flat.attach(g.device)
        hook = r.reducer.param_ready if r.reducer is not None else None
        # (deterministic mode: one stream - the weight-gradient launches share one workspace)
        side = side_stream(g.device) if (r.wgrad_on_side_stream and r.flat is not None and not K.deterministic()) else None
        if r.reducer is not None:
            r.reducer.wait_streams = [side] if side is not None else []
        gin = run_backward(r.prog, ctx.saved, g.contiguous(), want_wgrad=r.flat is not None, want_input_grad=ctx.want_x,
                           on_param_grad=hook, wgrad_stream=side, det_ws=r.det_workspace(g.device) if side is None else None,
                           x3_ws=r.x3_workspace(g.device), input_sink=getattr(r, "input_sink", None))
        ctx.saved = None
        return gin, None, None, None, None


_RUNNERS = weakref.WeakSet()


def trainable_runners(model):
    """Every conv-stack executor of `model` that owns a flat gradient buffer (built now if the module has not run yet): the backbone's,
    for the ContentAware backbone the feature extractor's and a trained mask predictor's, and a PerceptualHead's projection head
    (heads.PerceptualHead._ProjectionHead)."""
    out = []
    for m in model.modules():
        if not (hasattr(m, "_build") and hasattr(m, "__dict__") and "_runner" in m.__dict__):
            continue
        if getattr(m, "fix_mask", False):                 # (the all-ones mask predictor never runs)
            continue
        if m._runner is None:
            to_kernel_layout_(m)
            m._runner = m._build()
        if isinstance(m._runner, Runner) and m._runner.flat is not None:
            out.append(m._runner)
    return out


def set_stream_overlap(on, model=None):
    """Switch the side-stream overlap (weight gradients, the head's feature prefetch) of the Runners over `model`'s modules
    (all Runners when None) and of heads that hold a `prefetch_features` switch; returns nothing.  bench.py turns it off around
    its per-kernel timing leg."""
    mods = None if model is None else {id(m) for m in model.modules()}
    for r in list(_RUNNERS):
        if mods is None or id(r.module) in mods:
            r.wgrad_on_side_stream = bool(on)
    if model is not None:
        for m in model.modules():
            if hasattr(m, "prefetch_features"):
                m.prefetch_features = bool(on)


def invalidate_caches(model=None):
    """Drop every host-side copy derived from parameters / buffers (BatchNorm-folded weights, fragment-ordered packs, the
    transposed stem table) of the Runners over `model`'s modules (all Runners when None).  Needed wherever weights or
    running statistics change WITHOUT the eager forward's own bookkeeping seeing it: HIP-graph replays (no Python runs,
    fused Adam and the BatchNorm kernels bump no version counter) and the parameter broadcast of attach_reducer."""
    mods = None if model is None else {id(m) for m in model.modules()}
    for r in list(_RUNNERS):
        if mods is not None and id(r.module) not in mods:
            continue
        r._fold.clear()
        if r._packer is not None:
            r._packer.invalidate()
    K.invalidate_stem_tables()


class Runner:
    """Binds a Program to its nn.Module (parameter container) and, if trainable, a FlatGrads buffer."""

    def __init__(self, module, prog, trainable, precision="f32", fold_cache=None):
        _RUNNERS.add(self)
        self.module, self.prog = module, prog
        self.precision = K.PRECISION[str(precision).lower()]     # conv operand precision (0 fp32, 1 bf16 operands, 2 f32x3)
        # deterministic calls (include/bihome.h): a property of THIS Runner, fixed when it is built (kernels.set_deterministic /
        # BIHOME_DETERMINISTIC=1 give the default, `with kernels.det_scope(True): build_model(...)` a per-model choice) - the library has
        # no process-wide mode, two models of one process may differ
        self.det = K.deterministic()
        params = [p for p in module.parameters() if p.requires_grad]
        self.flat = FlatGrads(params) if (trainable and params) else None
        self.anchor = params[0] if (trainable and params) else None
        self._dummy = None
        self.reducer = None        # bihome_amd.ddp.FlatGradReducer when training data-parallel
        # eval-mode BatchNorm folding cache (run_forward / _folded); Runners over the SAME modules (the extractor's
        # 1- and 3-channel programs) share one dict so that a training forward through either invalidates both
        self._fold = fold_cache if fold_cache is not None else {}
        self.fold_bn = True                 # (tests switch it off to compare the folded and unfolded eval forwards)
        # second HIP stream for the weight-gradient launches (default since round 4: with three instead of six MFMA products per
        # product the 3x3 kernels are no longer matrix-pipe-bound and two streams fill each other's gaps: 15.5 -> 14.7 ms per step;
        # BIHOME_OVERLAP=0 or bench.py --no-overlap: one stream - per-kernel durations of rocprofv3 / the roofline leg are then those
        # of each kernel alone, which is how profiles/ and bench.py's roofline object are measured)
        self.wgrad_on_side_stream = os.environ.get("BIHOME_OVERLAP", "1") != "0"
        # fragment-ordered weight copies for the halo-tiled 3x3 kernel (csrc/conv3x3.hip PACKED; tests switch it off to compare with
        # the unpacked path)
        self.use_packer = True
        self._packer = None
        self._det_ws = None

    def det_workspace(self, device):
        """Deterministic mode: one workspace for the fixed-order split-K reduction of the weight gradients (every launch of the
        stride-1 fast path stores 2048 x 16 KB partial tiles)."""
        if not K.deterministic() or self.flat is None:
            return None
        if self._det_ws is None or self._det_ws.device != device or self._det_ws.numel() * 4 < DET_WS_BYTES:
            self._det_ws = torch.empty(DET_WS_BYTES // 4, dtype=torch.float32, device=device)
        return self._det_ws

    def x3_workspace(self, device):
        """'f32' arithmetic (precision 2): the 40 MB workspace the f32x3 weight-gradient kernel stores its <= 256 partial blocks
        of 147 KB in (wgrad_x3_reduce_kernel adds them in split order: those layers' gradients are bitwise reproducible)."""
        if K.deterministic():
            return self.det_workspace(device)
        if self.precision not in K.SPLIT_PIECES or self.flat is None:
            return None
        if self._det_ws is None or self._det_ws.device != device:
            self._det_ws = torch.empty(X3_WS_BYTES // 4, dtype=torch.float32, device=device)
        return self._det_ws

    def packer_for(self, device):
        if not self.use_packer:
            return None
        if self._packer is None or self._packer_dev != device:
            pk = K.packer_for_precision(self.precision)
            for op in self.prog.ops:
                if P.packs_weight(op, device):
                    pk.get(op.mod.weight)
            self._packer, self._packer_dev = pk, device
        return self._packer

    def __call__(self, x, groups):
        if not x.is_cuda:
            raise RuntimeError("bihome_amd runs on the MI355X only (input on %s): there is no CPU fallback; "
                               "use oracle/ for CPU checks" % x.device)
        anchor = self.anchor
        if anchor is None:
            if self._dummy is None or self._dummy.device != x.device:
                self._dummy = torch.zeros(1, device=x.device)
            anchor = self._dummy
        return NetFunction.apply(x, anchor, self, groups, torch.is_grad_enabled())
