"""The resident uint8 image bank on the device (bh_bank_gather_u8, csrc/bank.hip; bihome_amd/bank.py; GpuPairGenerator with bank=).
Every comparison is bitwise: the gather is an exact conversion of bytes to floats, and a generator that reads a bank must produce the
bits of the float path (a twin generator whose float `images` hold the same pixel values), which
test_head_kernels_gpu.py::test_gpu_pair_generator_matches_reference_fixture holds to the reference."""
import copy
import functools

import numpy as np
import pytest
import torch

import poisoned_alloc
from bihome_amd import configs

pytestmark = pytest.mark.gpu

N_BIG = 9400        # 240 x 320 x 3 bytes per image: image 9,321 is the first that starts past 2^31 bytes (9321 * 230400 = 2,147,558,400)


@functools.lru_cache(maxsize=None)
def pixels(n, h, w, seed=0):
    """uint8 [n,h,w,3] on the host, made once per shape and shared; callers do not modify it."""
    a = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


def as_planes(u8, idx):
    """The gather, restated with torch indexing: [count,3,h,w] float."""
    return u8[idx.long()].permute(0, 3, 1, 2).float().contiguous()


# ------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(24, 32), (23, 37), (240, 320)], ids=["24x32-vector", "23x37-scalar-odd-base", "240x320"])
def test_gather_is_exact(monkeypatch, h, w):
    from bihome_amd import bank as bank_module
    p = poisoned_alloc.poison(monkeypatch, bank_module)
    bank = bank_module.ImageBank(pixels(5, h, w).copy())
    idx = torch.tensor([4, 0, 2, 2, 0, 4, 1], dtype=torch.int32, device="cuda")
    out = bank.gather(idx)                                             # (allocated by bank.py through the poisoned torch.empty)
    assert "gather" in p.callers() and out.shape == (7, 3, h, w) and out.dtype == torch.float32
    want = as_planes(bank.data, idx)
    assert torch.equal(out, want)                                      # (no NaN of the poison left either: NaN != NaN)
    first = out.clone()
    again = bank.gather(idx)
    assert again.data_ptr() == out.data_ptr() and torch.equal(again, first)            # the staging buffer is reused; same bits
    # a caller's buffer; indices outside the bank read inside it (clamped)
    mine = bank_module.torch.empty((4, 3, h, w), dtype=torch.float32, device="cuda")
    wild = torch.tensor([-1, 5, 3, -2147483648], dtype=torch.int32, device="cuda")
    assert bank.gather(wild, out=mine) is mine
    assert torch.equal(mine, as_planes(bank.data, torch.tensor([0, 4, 3, 0], device="cuda")))
    assert p.verify() >= 2                                             # nothing written outside either output


def test_unaligned_views_take_the_scalar_path_with_the_same_bits():
    """A bank that starts on an odd byte and an output that starts 4 bytes off a 16-byte boundary (raw call: the wrapper only takes
    whole tensors): the width would allow the vector path, the addresses do not."""
    import ctypes
    from bihome_amd._lib import check, lib
    h, w = 24, 32
    raw = torch.zeros(1 + 5 * h * w * 3, dtype=torch.uint8, device="cuda")
    raw[1:] = torch.from_numpy(pixels(5, h, w).copy()).cuda().reshape(-1)
    u8 = raw[1:].view(5, h, w, 3)
    aligned = u8.clone()
    assert u8.data_ptr() % 4 == 1 and aligned.data_ptr() % 16 == 0
    idx = torch.tensor([3, 0, 4], dtype=torch.int32, device="cuda")
    buf = torch.full((1 + 3 * 3 * h * w + 1,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    pv = ctypes.c_void_p
    for bank_ptr, out_off in ((u8.data_ptr(), 0), (aligned.data_ptr(), 1), (u8.data_ptr(), 1)):
        buf.fill_(float("nan"))
        check(lib.bh_bank_gather_u8(pv(bank_ptr), pv(idx.data_ptr()), 3, 5, h, w, pv(buf.data_ptr() + 4 * out_off),
                                    pv(torch.cuda.current_stream().cuda_stream)), "bh_bank_gather_u8")
        got = buf[out_off:out_off + 3 * 3 * h * w].view(3, 3, h, w)
        assert torch.equal(got, as_planes(u8, idx))
        assert torch.isnan(buf[out_off + 3 * 3 * h * w:]).all() and torch.isnan(buf[:out_off]).all()


def test_offsets_are_64_bit():
    """The smallest bank whose last images start past 2^31 bytes: a 32-bit byte offset reads image 9,321 from the wrong place."""
    from bihome_amd.bank import ImageBank
    data = torch.randint(0, 256, (N_BIG, 240, 320, 3), dtype=torch.uint8, device="cuda")
    bank = ImageBank(data)
    assert bank.nbytes == N_BIG * 240 * 320 * 3 > 2 ** 31 and 9320 * 230400 < 2 ** 31 <= 9321 * 230400
    idx = torch.tensor([0, 9320, 9321, N_BIG - 1], dtype=torch.int32, device="cuda")
    out = bank.gather(idx)
    assert torch.equal(out, as_planes(bank.data, idx))
    # (random bytes: two images agree on 1/256 of their pixels) the four images differ, so an offset that wrapped would show
    assert not torch.equal(out[1], out[2]) and not torch.equal(out[0], out[3])


# ------------------------------------------------------------------------------------------------
# the generator on a bank
# ------------------------------------------------------------------------------------------------
GEN = dict(patch=32, rho=8)
CONFIGS = {
    "gray": dict(),
    "rgb": dict(channels=3),
    "pds-device-draws": dict(photometric_max_delta=32, photometric_draws="device"),
    "all_points": dict(target_gen="all_points"),
    "image": dict(image=True),
    "blobs": dict(blob_porosity=0.3, blobiness=0.5),
}


def pair(u8, seed, **kw):
    """(a generator on a bank of `u8`, its twin built the old way whose float images are the same pixel values)"""
    from bihome_amd.bank import ImageBank
    from bihome_amd.synth_gpu import GpuPairGenerator
    gen = GpuPairGenerator(seed=seed, bank=ImageBank(u8.copy()), **GEN, **kw)
    twin = GpuPairGenerator(n_images=u8.shape[0], seed=seed, **GEN, **kw)
    twin.images = torch.from_numpy(u8.copy()).cuda().permute(0, 3, 1, 2).float().contiguous()
    twin.h, twin.w = u8.shape[1], u8.shape[2]
    assert (gen.h, gen.w, gen.n_images) == (twin.h, twin.w, twin.n_images)
    return gen, twin


def assert_same_batch(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_on_a_bank_equals_the_float_path(name):
    gen, twin = pair(pixels(3, 80, 96, seed=1), 11, **CONFIGS[name])
    for _ in range(2):                                                 # (the second batch reuses the staging buffer)
        a, b = gen.next(4), twin.next(4)
        assert_same_batch(a, b)
    assert a["patch_1"].shape == (4, 3 if name == "rgb" else 1, 32, 32) and a["patch_1"].std().item() > 0.1
    if name == "image":
        assert a["image_1"].shape == (4, 1, 80, 96)


@pytest.mark.parametrize("where", ["host", "device"])
def test_given_indices_replace_the_index_draw_only(where):
    gen, twin = pair(pixels(3, 80, 96, seed=1), 12, photometric_max_delta=32, photometric_draws="device", image=True)
    i = np.array([2, 2, 0, 1])
    dev = torch.tensor(i, dtype=torch.int32, device="cuda")
    a = gen.next(4, idx=i if where == "host" else dev.long())
    drawn = twin.draw(4)
    assert_same_batch(a, twin.make(dev, *drawn[1:]))
    # ... and the generator's state went on as if it had drawn the indices itself
    assert_same_batch(gen.next(4), twin.next(4))


def test_epoch_follows_the_sampler(monkeypatch):
    from bihome_amd.bank import BankSampler, ImageBank
    from bihome_amd.synth_gpu import GpuPairGenerator
    u8 = np.ascontiguousarray(np.broadcast_to(np.arange(7, dtype=np.uint8)[:, None, None, None], (7, 80, 96, 3)))
    bank = ImageBank(u8)                                               # every pixel of image k holds k
    gen = GpuPairGenerator(seed=3, bank=bank, **GEN)
    staged, gather = [], bank.gather

    def spy(idx, out=None):
        r = gather(idx, out)
        staged.append(r.clone())
        return r
    monkeypatch.setattr(bank, "gather", spy)
    sampler, restart = BankSampler(len(bank), 4, 10, seed=21), BankSampler(len(bank), 4, 10, seed=21)
    want = list(restart) + list(restart)                               # two epochs of the same seed
    batches = list(gen.epoch(sampler)) + list(gen.epoch(sampler))      # (the sampler's state continues: the second epoch is another order)
    assert len(sampler) == 2 and len(batches) == len(staged) == len(want) == 4
    for batch, images, idx in zip(batches, staged, want):
        assert batch["patch_1"].shape == (4, 1, 32, 32)
        k = torch.tensor(idx, dtype=torch.float32, device="cuda")
        assert torch.equal(images, k[:, None, None, None].expand(4, 3, 80, 96))
        # a constant image of value k: patch_1 is one standardised constant per sample, increasing with k
        v = batch["patch_1"][:, 0, 0, 0]
        assert torch.equal(batch["patch_1"], v[:, None, None, None].expand(4, 1, 32, 32))
        assert torch.equal(k[:, None] < k[None, :], v[:, None] < v[None, :])
    # an index outside the bank that arrives from the host is refused before anything is launched
    n = len(staged)
    for bad in ([0, 1, 7, 0], [0, -1, 0, 0]):
        with pytest.raises(ValueError):
            gen.next(4, idx=bad)
    assert len(staged) == n


@pytest.mark.parametrize("name", ["zeng-bihome-pds", "nguyen-orig"])
def test_from_config_with_a_bank(name):
    from bihome_amd.bank import ImageBank
    from bihome_amd.synth_gpu import GpuPairGenerator, batch_spec
    cfg = copy.deepcopy(configs.get(name))
    cfg["DATA"]["PATCH_SIZE"], cfg["DATA"]["RHO"] = 32, 8
    bank = ImageBank(pixels(3, 80, 96, seed=1).copy())
    gen = GpuPairGenerator.from_config(cfg, bank=bank)
    assert gen.bank is bank and (gen.n_images, gen.h, gen.w) == (3, 80, 96) and gen.photometric_draws == "device"
    spec = batch_spec(cfg)
    assert (spec["patch"], spec["rho"]) == (32, 8)
    batch = gen.next(4)
    want = {"patch_1", "patch_2", "delta"} | ({"target"} if spec["target_gen"] else set()) | \
        ({"corners"} if spec["corners"] else set()) | ({"image_1"} if spec["image"] else set())
    assert set(batch) == want
    assert batch["patch_1"].shape == batch["patch_2"].shape == (4, spec["channels"], 32, 32) and batch["delta"].shape == (4, 4, 2)
    if name == "nguyen-orig":
        assert batch["image_1"].shape == (4, 1, 80, 96) and batch["corners"].shape == (4, 4, 2)
    for v in batch.values():
        assert torch.isfinite(v).all()
