"""A stand-in for the `torch` module that poisons what `torch.empty` hands out and fences every allocation with red zones.

The wrappers of bihome_amd/kernels.py (and the heads, net.py, step.py, synth_gpu.py) allocate outputs, scratch and workspaces with
`torch.empty`.  In a fresh process the caching allocator mostly hands out zero pages, so a kernel that reads a scratch entry before it
writes it, relies on a zeroed buffer it was not given, leaves part of an "overwritten" output unwritten or writes past the size its
size query promised passes every parity test - and is wrong in a long run, where blocks are recycled.  `poison(monkeypatch, module...)`
replaces the `torch` global of the listed modules by one `Poisoned` object: their code runs unchanged and every `torch.empty(...)` /
`torch.empty_like(...)` gets

    [ red zone, 4096 bytes | the requested elements | red zone, 4096 bytes ]

filled throughout - NaN for floating dtypes, 1 for integer / byte / bool dtypes (not the zero of a fresh page, yet in range wherever a
kernel might take a stale element for an index or a count) - and returned as the interior view, which starts 4096 bytes (a multiple of
512) into the allocator's block: vector and buffer loads see the alignment they see from torch.empty.  `torch.zeros` / `zeros_like` keep
their zero interior between the same red zones.  `verify()` holds every red zone against its fill bit for bit.

Only device tensors are fenced (CPU requests pass through) unless the object is built with cpu=True - the self-test of this module in
test_buffer_contracts_cpu.py."""
import sys

import torch

RED_ZONE_BYTES = 4096
ALIGN_BYTES = 512
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _pattern(dtype):
    """(integer dtype of the same width, the fill element's bits as that integer): the fill is written and compared as integers, so a NaN
    is one fixed bit pattern and `verify` is a bitwise comparison."""
    if dtype.is_complex:
        raise NotImplementedError("poisoned_alloc: complex dtypes")
    itype = _INT_VIEW[torch.empty((), dtype=dtype).element_size()]
    one = torch.full((1,), float("nan") if dtype.is_floating_point else 1, dtype=dtype)
    return itype, int(one.view(itype).item())


class Record:
    __slots__ = ("caller", "module", "shape", "dtype", "block", "front", "n", "itype", "bits")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def zones(self):
        """(side, integer view of the zone) for the two red zones."""
        ib = self.block.view(self.itype)
        return (("front", ib[:self.front]), ("behind", ib[self.front + self.n:]))


class Poisoned:
    """Forwards every attribute to `torch` except empty, empty_like, zeros and zeros_like."""

    def __init__(self, cpu=False):
        self._cpu = bool(cpu)
        self._records = []
        self._callers = set()
        self._modules = {}          # caller -> set of module names

    def __getattr__(self, name):
        return getattr(torch, name)

    # ---- the four replaced factories ----------------------------------------------------------
    def empty(self, *args, **kw):
        return self._alloc(torch.empty(*args, **dict(kw, device="meta")), kw.get("device"), kw, False, sys._getframe(1))

    def zeros(self, *args, **kw):
        return self._alloc(torch.zeros(*args, **dict(kw, device="meta")), kw.get("device"), kw, True, sys._getframe(1))

    def empty_like(self, t, **kw):
        return self._alloc(torch.empty_like(t, **dict(kw, device="meta")), kw.get("device", t.device), kw, False, sys._getframe(1))

    def zeros_like(self, t, **kw):
        return self._alloc(torch.zeros_like(t, **dict(kw, device="meta")), kw.get("device", t.device), kw, True, sys._getframe(1))

    # ---- allocation ----------------------------------------------------------------------------
    def _alloc(self, meta, device, kw, zero, frame):
        """meta: the tensor torch would have made, on the meta device - torch's own parsing of sizes, dtype defaults and memory formats."""
        device = torch.device(device) if device is not None else torch.device("cpu")
        if kw.get("out") is not None or kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided:
            raise NotImplementedError("poisoned_alloc: out= / pin_memory / layout requests")
        n = meta.numel()
        if n == 0 or (device.type == "cpu" and not self._cpu):
            real = torch.zeros_like(meta, device=device) if zero else torch.empty_like(meta, device=device)
            return real.requires_grad_(True) if kw.get("requires_grad") else real
        shape, strides, dtype = tuple(meta.shape), tuple(meta.stride()), meta.dtype
        assert 1 + sum((s - 1) * st for s, st in zip(shape, strides)) == n, "poisoned_alloc: not a dense layout %s / %s" % (shape, strides)
        size = meta.element_size()
        assert RED_ZONE_BYTES % size == 0 and RED_ZONE_BYTES % ALIGN_BYTES == 0
        front = RED_ZONE_BYTES // size
        itype, bits = _pattern(dtype)
        block = torch.empty(front + n + front, dtype=dtype, device=device)
        block.view(itype).fill_(bits)
        inner = block[front:front + n]
        if zero:
            inner.zero_()
        out = inner.as_strided(shape, strides, inner.storage_offset())
        assert (out.data_ptr() - block.data_ptr()) % ALIGN_BYTES == 0 and out.data_ptr() - block.data_ptr() == RED_ZONE_BYTES
        caller, module = frame.f_code.co_name, frame.f_globals.get("__name__", "?")
        self._callers.add(caller)
        self._modules.setdefault(caller, set()).add(module)
        self._records.append(Record(caller=caller, module=module, shape=shape, dtype=dtype, block=block, front=front, n=n, itype=itype, bits=bits))
        return out.requires_grad_(True) if kw.get("requires_grad") else out

    # ---- inspection ----------------------------------------------------------------------------
    def callers(self):
        """Names of the functions that allocated through this object."""
        return set(self._callers)

    def modules_of(self, caller):
        return set(self._modules.get(caller, ()))

    def __len__(self):
        return len(self._records)

    def verify(self):
        """Synchronise and assert that every red zone recorded so far still holds its fill, bit for bit; the records checked are released
        (so is their memory), the callers' names are kept."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        records, self._records = self._records, []
        flags = {}
        for i, r in enumerate(records):                     # (one small comparison per zone, queued; fetched once per device below)
            for side, z in r.zones():
                flags.setdefault(z.device, []).append(((i, side), (z != r.bits).any()))
        damaged = []
        for dev, fl in flags.items():
            hit = torch.stack([f for _, f in fl]).cpu().tolist()
            damaged += [key for (key, _), h in zip(fl, hit) if h]
        report = []
        for i, side in damaged:
            r = records[i]
            z = dict(r.zones())[side]
            off = int((z != r.bits).nonzero()[0].item())
            # first damaged element, in elements relative to the interior: negative in front of it, >= numel behind it
            rel = off - r.front if side == "front" else r.n + off
            report.append("%s (%s): %s %s, red zone %s damaged first at element %d of the zone (offset %d from the interior's start, %d bytes)"
                          % (r.caller, r.module, tuple(r.shape), r.dtype, side, off, rel, rel * (RED_ZONE_BYTES // r.front)))
        assert not report, "%d of %d red zones written to:\n  %s" % (len(report), 2 * len(records), "\n  ".join(report))
        return len(records)


def poison(monkeypatch, *modules, cpu=False):
    """Install ONE Poisoned object as the `torch` global of each given module (only those: weights.py, the optimizer and the reference
    code of the tests keep the real one) and return it; monkeypatch restores the modules when the test ends."""
    p = Poisoned(cpu=cpu)
    for m in modules:
        assert getattr(m, "torch", None) is torch or isinstance(getattr(m, "torch", None), Poisoned), "%s has no `torch` global" % m.__name__
        monkeypatch.setattr(m, "torch", p)
    return p
