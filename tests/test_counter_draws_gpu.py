"""Counter-based draws on the device: every array of bh_synth_draw bitwise against the numpy oracle `synth.counter_draws`, the buffer
contract (poisoned, red-zoned outputs; refusals touch nothing), and the generator's counter mode: resume, rank independence, idx=, and
the untouched torch mode."""
import ctypes

import numpy as np
import pytest
import torch

import poisoned_alloc
from bihome_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ("img_idx", "origin", "delta", "photo", "noise", "other")
SEED = 42


def buffers(p, B, P, photo=True, blobs=False):
    """The outputs of one call from the poisoned allocator (NaN / 1 fill between two red zones each)."""
    out = {"img_idx": p.empty(B, dtype=torch.int32, device="cuda"), "origin": p.empty(B, 2, dtype=torch.float32, device="cuda"),
           "delta": p.empty(B, 4, 2, dtype=torch.float32, device="cuda"), "photo": None, "noise": None, "other": None}
    if photo:
        out["photo"] = p.empty(B, 2, 6, dtype=torch.float32, device="cuda")
    if blobs:
        out["noise"], out["other"] = p.empty(B, P, P, dtype=torch.float32, device="cuda"), p.empty(B, dtype=torch.int32, device="cuda")
    return out


def device_draw(p, seed, first, B, n_images, geom, md, photo=True, blobs=False):
    from bihome_amd import kernels as K
    P, rho, h, w = geom
    out = buffers(p, B, P, photo, blobs)
    K.synth_draw(seed, first, n_images, h, w, P, rho, md, *(out[k] for k in KEYS))
    return out


def assert_bits(out, want):
    for k in KEYS:
        if out[k] is None:
            continue
        got = out[k].cpu().numpy()
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
        assert got.tobytes() == want[k].tobytes(), (k, got.ravel()[:8], want[k].ravel()[:8])


G_COCO, G_ODD, G_TIGHT, G_FULL = (32, 8, 240, 320), (17, 1, 19, 23), (16, 4, 24, 24), (128, 32, 240, 320)
CASES = [
    # B, first, n_images, (P, rho, Hs, Ws), max_delta, photo, blobs
    (1, 0, 1, G_COCO, 0, True, False),
    (5, 2 ** 32 - 3, 3, G_COCO, 32, True, True),
    (65, 2 ** 63, 2 ** 31 - 1, G_COCO, 32, True, False),
    (65, 0, 3, G_ODD, 32, True, False),
    (3, 2 ** 32 - 3, 2 ** 31 - 1, G_ODD, 0, True, True),             # P * P % 4 != 0: the scalar noise stores
    (5, 2 ** 63, 3, G_TIGHT, 0, True, True),
    (2, 2 ** 32 - 3, 1, G_TIGHT, 32, True, True),
    (2, 0, 3, G_COCO, 32, False, True),                               # photo = NULL
    (5, 0, 3, G_COCO, 0, False, False),                               # photo = noise = other = NULL
    (1, 2 ** 63, 3, G_TIGHT, 32, False, False),
    (2, 2 ** 63, 3, G_FULL, 32, True, True),                          # P = 128
]


@pytest.mark.parametrize("B,first,n_images,geom,md,photo,blobs", CASES,
                         ids=["B%d-first%x-ni%d-P%d-md%d%s%s" % (c[0], c[1], c[2], c[3][0], c[4], "" if c[5] else "-nophoto", "-blobs" if c[6] else "")
                              for c in CASES])
def test_bitwise_against_the_oracle(B, first, n_images, geom, md, photo, blobs):
    P, rho, h, w = geom
    want = synth.counter_draws(SEED, first, B, n_images, h, w, P, rho, md, blobs=blobs)
    p = poisoned_alloc.Poisoned()
    out = device_draw(p, SEED, first, B, n_images, geom, md, photo, blobs)
    assert_bits(out, want)                                            # (bitwise: so no element kept its poison either)
    assert p.verify() == sum(v is not None for v in out.values())
    again = device_draw(p, SEED, first, B, n_images, geom, md, photo, blobs)
    for k in KEYS:
        assert out[k] is None or torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k
    p.verify()


def test_another_seed_and_an_unaligned_noise_plane():
    """Seeds up to 2^64 - 1; a noise plane that starts 4 bytes past a 16-byte boundary takes the scalar stores: the same bits, and the
    float in front of it and the one behind it keep their poison."""
    from bihome_amd import kernels as K
    seed, B, (P, rho, h, w) = 2 ** 64 - 1, 3, G_TIGHT
    want = synth.counter_draws(seed, 7, B, 5, h, w, P, rho, 32, blobs=True)
    p = poisoned_alloc.Poisoned()
    out = buffers(p, B, P, True, True)
    raw = p.empty(B * P * P + 2, dtype=torch.float32, device="cuda")
    out["noise"] = raw[1:1 + B * P * P].view(B, P, P)
    assert out["noise"].data_ptr() % 16 == 4
    K.synth_draw(seed, 7, 5, h, w, P, rho, 32, *(out[k] for k in KEYS))
    assert_bits(out, want)
    assert torch.isnan(raw[0]) and torch.isnan(raw[-1])
    p.verify()


def test_refusals_touch_nothing():
    from bihome_amd._lib import lib
    p = poisoned_alloc.Poisoned()
    P, rho, h, w = G_TIGHT
    B = 4
    out = buffers(p, B, P, True, True)
    before = {k: out[k].view(torch.int32).clone() for k in KEYS}
    ptr = {k: ctypes.c_void_p(out[k].data_ptr()) for k in KEYS}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B=B, n_images=3, h=h, w=w, P=P, rho=rho, **drop):
        a = [None if drop.get(k) else ptr[k] for k in KEYS]
        return lib.bh_synth_draw(SEED, 0, B, n_images, h, w, P, rho, 32.0, *a, stream)

    bad = [dict(img_idx=True), dict(origin=True), dict(delta=True), dict(B=-1), dict(n_images=0), dict(rho=0), dict(P=0),
           dict(h=P + 2 * rho - 1), dict(w=P + 2 * rho - 1), dict(noise=True), dict(other=True), dict(B=1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k].view(torch.int32), before[k]), k
    assert call(B=0) == 0                                             # nothing launched
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k].view(torch.int32), before[k]), k
    assert call() == 0 and call(photo=True) == 0 and call(B=1, noise=True, other=True) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out["noise"]).any() and not torch.isnan(out["photo"]).any()
    p.verify()


# ---- the generator -------------------------------------------------------------------------------------------------------------
GEN = dict(n_images=3, patch=32, rho=8, seed=11, photometric_max_delta=32, corners=True, target_gen="all_points")


def same_batch(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_counter_draw_is_the_oracle_and_moves_the_position(monkeypatch):
    from bihome_amd import synth_gpu
    from bihome_amd.synth_gpu import GpuPairGenerator
    g = GpuPairGenerator(draws="counter", blob_porosity=0.3, blobiness=1.0, **GEN)

    def forbidden(*a, **k):
        raise AssertionError("counter mode made a torch draw or a record tensor")
    monkeypatch.setattr(synth_gpu, "photometric_records", forbidden)
    p = poisoned_alloc.poison(monkeypatch, synth_gpu)
    for name in ("rand", "randint"):
        monkeypatch.setattr(p, name, forbidden, raising=False)
    for first, B in ((0, 5), (5, 3)):
        idx, origin, delta, photo, (noise, other) = g.draw(B)
        want = synth.counter_draws(11, first, B, 3, g.h, g.w, 32, 8, 32, blobs=True)
        assert_bits({"img_idx": idx, "origin": origin, "delta": delta, "photo": photo.view(B, 2, 6), "noise": noise, "other": other}, want)
    assert g.position == 8 and "_draw_counter" in p.callers()
    far = g.draw(2, first=2 ** 63)                                    # an explicit position leaves the generator's alone
    assert g.position == 8
    assert far[2].cpu().numpy().tobytes() == synth.counter_draws(11, 2 ** 63, 2, 3, g.h, g.w, 32, 8, 32)["delta"].tobytes()
    p.verify()
    # without distortion there is no record, as in torch mode
    assert GpuPairGenerator(draws="counter", **dict(GEN, photometric_max_delta=0)).draw(2)[3] is None


def test_resume_from_a_state_dict():
    from bihome_amd.synth_gpu import GpuPairGenerator
    kw = dict(draws="counter", blob_porosity=0.3, blobiness=1.0, **GEN)
    g1 = GpuPairGenerator(**kw)
    first = g1.next(4)
    state = g1.state_dict()
    assert state == {"draws": "counter", "seed": 11, "position": 4}
    second = g1.next(4)
    g2 = GpuPairGenerator(**kw)
    g2.load_state_dict(state)
    same_batch(g2.next(4), second)
    assert not torch.equal(first["patch_1"], second["patch_1"]) and g2.state_dict() == g1.state_dict()


def test_ranks_split_one_global_batch():
    from bihome_amd.synth_gpu import GpuPairGenerator
    one = GpuPairGenerator(draws="counter", **GEN)
    ranks = [GpuPairGenerator(draws="counter", rank=r, world=2, **GEN) for r in (0, 1)]
    for _ in range(2):                                                # (the second round: position moved on by world * B)
        whole = one.next(6)
        parts = [g.next(3) for g in ranks]
        for k in ("patch_1", "patch_2", "delta", "corners", "target"):
            assert torch.equal(torch.cat([parts[0][k], parts[1][k]]), whole[k]), k
    assert one.position == 12 and [g.position for g in ranks] == [12, 12]
    assert not torch.equal(parts[0]["delta"], parts[1]["delta"])


def test_bank_and_callers_indices():
    from bihome_amd.bank import ImageBank
    from bihome_amd.synth_gpu import GpuPairGenerator
    px = np.random.RandomState(0).randint(0, 256, (5, 48, 56, 3)).astype(np.uint8)
    kw = dict(patch=32, rho=8, seed=11, photometric_max_delta=32, draws="counter", corners=True)
    mine = [4, 0, 2, 2]
    a = GpuPairGenerator(bank=ImageBank(px), **kw)
    b = GpuPairGenerator(bank=ImageBank(px), **kw)
    da, db = a.draw(4), b.draw(4, idx=mine)
    assert db[0].dtype == torch.int32 and db[0].tolist() == mine
    want = synth.counter_draws(11, 0, 4, 5, 48, 56, 32, 8, 32)
    assert da[0].cpu().numpy().tobytes() == want["img_idx"].tobytes()
    for x, y in zip(da[1:], db[1:]):
        assert torch.equal(x, y)                                      # origin, delta, photo: unchanged by idx=
    assert a.position == b.position == 4
    batch = b.make(*db)
    # sample 1 is image 0 of the bank: the same sample drawn with every index 0 has the same patches
    c = GpuPairGenerator(bank=ImageBank(px), **kw)
    ref = c.make(*c.draw(4, idx=[0, 0, 0, 0]))
    assert torch.equal(batch["patch_1"][1], ref["patch_1"][1]) and torch.equal(batch["patch_2"][1], ref["patch_2"][1])
    assert not torch.equal(batch["patch_1"][0], ref["patch_1"][0])
    assert torch.equal(batch["corners"], ref["corners"]) and torch.isfinite(batch["patch_2"]).all()
    with pytest.raises(ValueError):
        b.draw(4, idx=[0, 1, 2, 5])


@pytest.mark.parametrize("explicit", [False, True], ids=["default", "draws=torch"])
def test_torch_mode_is_what_it_was(explicit):
    """draws='torch' (the default): draw() restated as it is without the counter mode - the same calls on a device generator of the same
    seed, device-drawn records, blob draws last - gives the same bits, call after call, and make() the same batch."""
    from bihome_amd.synth_gpu import GpuPairGenerator, photometric_records
    seed, B, patch, rho, md = 12, 6, 32, 8, 32
    kw = dict(n_images=3, patch=patch, rho=rho, seed=seed, photometric_max_delta=md, photometric_draws="device", blob_porosity=0.3,
              blobiness=1.0)
    gen = GpuPairGenerator(draws="torch", **kw) if explicit else GpuPairGenerator(**kw)
    twin = GpuPairGenerator(**kw)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    half = patch // 2
    for _ in range(2):
        idx = torch.randint(0, 3, (B,), generator=g, device="cuda", dtype=torch.int32)
        px = torch.randint(rho + half, gen.w - rho - half + 1, (B,), generator=g, device="cuda")
        py = torch.randint(rho + half, gen.h - rho - half + 1, (B,), generator=g, device="cuda")
        origin = torch.stack([px - half, py - half], 1).to(torch.float32).contiguous()
        delta = torch.randint(-rho, rho, (B, 4, 2), generator=g, device="cuda").to(torch.float32).contiguous()
        photo = photometric_records(torch.rand((B, 2, 11), generator=g, device="cuda"), md).reshape(B, 12).contiguous()
        noise = torch.rand((B, patch, patch), generator=g, device="cuda")
        r = torch.randint(0, B - 1, (B,), generator=g, device="cuda")
        other = (r + (r >= torch.arange(B, device="cuda"))).to(torch.int32)
        want = twin.make(idx, origin, delta, photo, (noise, other))
        got = gen.draw(B)
        for x, y in zip(got[:4] + got[4], (idx, origin, delta, photo, noise, other)):
            assert x.dtype == y.dtype and torch.equal(x, y)
        same_batch(gen.make(*got), want)
