"""tests/poisoned_alloc.py on CPU tensors, and the census that keeps tests/test_buffer_contracts_gpu.py complete: every function of
bihome_amd/kernels.py that calls torch.empty / torch.empty_like is either run under the shim by a case there (COVERED_BY) or listed with a
reason (EXEMPT, five names at the most) - a wrapper added later fails here until someone poisons it."""
import ast
import os

import pytest
import torch

import poisoned_alloc
from poisoned_alloc import ALIGN_BYTES, RED_ZONE_BYTES, Poisoned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.float64, torch.float16, torch.int64, torch.int32, torch.uint8, torch.bool]


def _bytes(t):
    """The bytes of the storage `t` views, as a uint8 tensor, and t's offset into it in bytes."""
    st = t.untyped_storage()
    return torch.tensor([], dtype=torch.uint8).set_(st, 0, (st.nbytes(),)), t.storage_offset() * t.element_size()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_empty_is_poisoned_aligned_and_shaped(dtype):
    p = Poisoned(cpu=True)
    for t in (p.empty(3, 5, dtype=dtype), p.empty((3, 5), dtype=dtype, device="cpu"), p.empty(torch.Size([3, 5]), dtype=dtype),
              p.empty_like(torch.zeros(3, 5, dtype=dtype))):
        assert tuple(t.shape) == (3, 5) and t.dtype == dtype and t.is_contiguous()
        raw, off = _bytes(t)
        assert off == RED_ZONE_BYTES and off % ALIGN_BYTES == 0 and raw.numel() == 2 * RED_ZONE_BYTES + 15 * t.element_size()
        if dtype.is_floating_point:
            assert torch.isnan(t).all()
        else:
            assert (t.to(torch.int64) == 1).all()
    assert p.callers() == {"test_empty_is_poisoned_aligned_and_shaped"} and p.modules_of("test_empty_is_poisoned_aligned_and_shaped") == {__name__}
    assert len(p) == 4 and p.verify() == 4 and len(p) == 0


def test_default_dtype_strided_like_and_requires_grad():
    p = Poisoned(cpu=True)
    assert p.empty(7).dtype == torch.get_default_dtype()
    cl = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    like = p.empty_like(cl)                                  # torch.empty_like keeps a dense layout: so does the stand-in
    assert like.stride() == cl.stride() and torch.isnan(like).all()
    assert p.empty_like(cl, dtype=torch.int32).dtype == torch.int32
    assert p.zeros(4, dtype=torch.float64, requires_grad=True).requires_grad
    p.verify()


def test_zeros_keep_a_zero_interior_between_red_zones():
    p = Poisoned(cpu=True)
    for t in (p.zeros(4, 2), p.zeros_like(torch.ones(4, 2)), p.zeros(8, dtype=torch.uint8)):
        assert (t == 0).all()
        raw, off = _bytes(t)
        assert off == RED_ZONE_BYTES and (raw[:off] != 0).any() and (raw[off + t.numel() * t.element_size():] != 0).any()
    assert p.verify() == 3


def test_passes_through_what_it_does_not_fence():
    p = Poisoned()                                            # (device tensors only)
    t = p.empty(5)
    assert _bytes(t)[0].numel() == 20 and len(p) == 0 and p.callers() == set()
    q = Poisoned(cpu=True)
    assert q.empty(0, 3).shape == (0, 3) and q.zeros(0).numel() == 0 and len(q) == 0      # zero-element requests
    assert q.float32 is torch.float32 and q.nn is torch.nn and q.tensor is torch.tensor and q.cuda is torch.cuda


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.uint8], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("side", ["front", "behind"])
def test_one_element_outside_the_interior_is_reported(side, dtype):
    p = Poisoned(cpu=True)
    keep = p.empty(6, dtype=dtype)
    t = p.empty(2, 3, dtype=dtype)
    base = torch.tensor([], dtype=dtype).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes() // t.element_size(),))
    at = t.storage_offset() - 1 if side == "front" else t.storage_offset() + t.numel()
    base[at] = 3
    with pytest.raises(AssertionError) as e:
        p.verify()
    msg = str(e.value)
    assert "red zone %s" % side in msg and "test_one_element_outside_the_interior_is_reported" in msg and "(2, 3)" in msg
    assert ("offset %d from" % (-1 if side == "front" else 6)) in msg and "1 of 4 red zones" in msg, msg
    del keep


def test_a_nan_of_another_bit_pattern_is_damage():
    p = Poisoned(cpu=True)
    t = p.empty(4)
    raw, off = _bytes(t)
    raw[off - 4:off] = torch.tensor([1, 0, 0xC0, 0x7F], dtype=torch.uint8)      # still a NaN, one bit apart: bit for bit means bit for bit
    with pytest.raises(AssertionError, match="front"):
        p.verify()


def test_interior_writes_pass():
    p = Poisoned(cpu=True)
    a, b, c = p.empty(1000), p.empty(3, dtype=torch.int32), p.zeros(17, dtype=torch.float64)
    a.fill_(2.0), b.fill_(-5), c.fill_(float("inf"))
    assert p.verify() == 3


def test_poison_installs_one_object_on_the_listed_modules_only(monkeypatch):
    import types
    a, b, c = types.ModuleType("a"), types.ModuleType("b"), types.ModuleType("c")
    for m in (a, b, c):
        m.torch = torch
        exec("def make():\n    return torch.empty(3)", m.__dict__)
    with monkeypatch.context() as mp:
        p = poisoned_alloc.poison(mp, a, b, cpu=True)
        assert a.torch is p and b.torch is p and c.torch is torch
        assert torch.isnan(a.make()).all() and torch.isnan(b.make()).all() and len(p) == 2
        c.make()
        assert len(p) == 2 and p.callers() == {"make"} and p.modules_of("make") == {"a", "b"}
        p.verify()
    assert a.torch is torch and b.torch is torch


# ------------------------------------------------------------------------------------------------
# the coverage census
# ------------------------------------------------------------------------------------------------
def allocating_functions(path):
    """Names of the functions (methods included) whose body calls torch.empty / torch.empty_like."""
    tree = ast.parse(open(path).read())
    names = set()
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for node in ast.walk(fn):
                f = getattr(node, "func", None)
                if (isinstance(node, ast.Call) and isinstance(f, ast.Attribute) and f.attr in ("empty", "empty_like")
                        and isinstance(f.value, ast.Name) and f.value.id == "torch"):
                    names.add(fn.name)
    return names


def test_every_allocating_wrapper_is_covered_or_exempt():
    import test_buffer_contracts_gpu as G
    census = allocating_functions(os.path.join(ROOT, "bihome_amd", "kernels.py"))
    assert len(census) > 40                                   # (the parse found the wrappers)
    assert len(G.EXEMPT) <= 5 and all(isinstance(r, str) and r.strip() and "\n" not in r for r in G.EXEMPT.values()), G.EXEMPT
    assert not set(G.COVERED_BY) & set(G.EXEMPT)
    listed = set(G.COVERED_BY) | set(G.EXEMPT)
    assert listed == census, "not covered: %s; listed but not allocating: %s" % (sorted(census - listed), sorted(listed - census))
    ids = {c[0] for c in G.CASES}
    assert len(ids) == len(G.CASES) and set(G.COVERED_BY.values()) <= ids
