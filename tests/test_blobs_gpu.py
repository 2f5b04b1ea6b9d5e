"""Occlusion blobs of the pair generator on the device (bh_synth_blobs, csrc/blobs.hip; K.synth_blobs; GpuPairGenerator with
blob_porosity / blobiness): the reference's CollatorWithBlobs (src/data/transforms.py:746-799).  The oracle is the float64 restatement
bihome_amd/synth.py blob_field / apply_blobs, which tests/test_blobs_cpu.py pins against scipy and against the fixture recorded from the
reference's own collator.  Noise comes from RandomState(0) as float32 values, so both sides see the same numbers.

Field bound: max(4 s, 1e-6), s = the float32 numpy restatement's own maximum deviation from float64 on the same noise (printed); the
factor 4 allows for a different summation order and fused multiply-adds.  Mask rule: equal to the reference mask on every pixel whose
float64 field is at least 1e-3 away from the porosity (the field bound is asserted to be below that), with at most 1 % of the pixels
inside the band (asserted on the reference alone)."""
import functools

import numpy as np
import pytest
import torch

from bihome_amd import configs, synth
from bihome_amd.weights import load_synthetic

pytestmark = pytest.mark.gpu

BAND = 1e-3
# (P, blobiness, B, C): radius == P, every tap row reflects | three channels | the LDS-capacity shape, radius 64 | the shape of
# zeng-bihome-rgb256, beyond LDS (three launches through global scratch)
SHAPES = [(32, 0.1, 2, 1), (32, 0.5, 2, 3), (128, 0.2, 3, 1), (256, 1.0, 2, 3)]


@functools.lru_cache(maxsize=None)
def reference(P, blobiness, B):
    """(noise float32 [B,P,P], u64 [B,P,P], s): computed once per shape and shared; callers do not modify it."""
    noise = np.random.RandomState(0).rand(B, P, P).astype(np.float32)
    u64 = np.stack([synth.blob_field(n.astype(np.float64), blobiness) for n in noise])
    u32 = np.stack([synth.blob_field(n, blobiness) for n in noise])
    assert u32.dtype == np.float32
    s = float(np.abs(u32.astype(np.float64) - u64).max())
    for a in (noise, u64):
        a.setflags(write=False)
    return noise, u64, s


def patches(B, C, P, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, P, P, generator=g).cuda(), torch.randn(B, C, P, P, generator=g).cuda()


def other_of(B, seed=2):
    r = np.random.RandomState(seed).randint(0, B - 1, B)
    return torch.tensor(r + (r >= np.arange(B)), dtype=torch.int32).cuda()


def run(noise, other, p1, p2, P, blobiness, porosity, want_field=True):
    """K.synth_blobs (through synth_gpu.apply_blobs, which allocates its outputs) on a copy of p2 -> (mask, field, new p2)."""
    from bihome_amd import synth_gpu
    out = p2.clone()
    mask, field = synth_gpu.apply_blobs(torch.tensor(np.array(noise)).cuda(), other, p1, out, synth.blob_sigma(P, blobiness), porosity,
                                        want_field=want_field)
    torch.cuda.synchronize()
    return mask, field, out


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_composite(mask, other, p1, p2_old, p2_new):
    """patch_2 is bitwise patch_1[other] under the mask and bitwise its old value elsewhere, in every channel."""
    m = (mask != 0)[:, None].expand_as(p2_new)
    assert ((mask == 0) | (mask == 1)).all()
    want = torch.where(m, bits(p1[other.long()]), bits(p2_old))
    assert torch.equal(bits(p2_new), want)


@pytest.mark.parametrize("P,blobiness,B,C", SHAPES)
def test_field_accuracy(P, blobiness, B, C):
    noise, u64, s = reference(P, blobiness, B)
    bound = max(4 * s, 1e-6)
    p1, p2 = patches(B, C, P)
    mask, field, _ = run(noise, other_of(B), p1, p2, P, blobiness, 0.3)
    f = field.cpu().numpy().astype(np.float64)
    err = np.abs(f - u64).max()
    print("P %d blobiness %g: float32 restatement s = %.3e, bound %.3e, kernel max |field - u64| = %.3e" % (P, blobiness, s, bound, err))
    assert np.isfinite(f).all() and f.min() == 0.0 and f.max() == 1.0
    assert err <= bound


@pytest.mark.parametrize("porosity", [0.1, 0.3, 0.5])
@pytest.mark.parametrize("P,blobiness,B,C", SHAPES)
def test_mask_agreement(P, blobiness, B, C, porosity):
    noise, u64, s = reference(P, blobiness, B)
    assert max(4 * s, 1e-6) < BAND
    decided = np.abs(u64 - porosity) >= BAND
    share = 1.0 - decided.mean()
    print("P %d blobiness %g porosity %g: %.3f %% of the pixels within %g of the threshold" % (P, blobiness, porosity, 100 * share, BAND))
    assert share <= 0.01                                             # precondition, on the reference alone
    p1, p2 = patches(B, C, P)
    other = other_of(B)
    mask, _, out = run(noise, other, p1, p2, P, blobiness, porosity, want_field=False)
    m = mask.cpu().numpy() != 0
    assert np.array_equal(m[decided], (u64 < porosity)[decided])
    assert m.any() and not m.all()
    assert_composite(mask, other, p1, p2, out)


@pytest.mark.parametrize("P,blobiness,B,C", SHAPES)
def test_porosity_edges(P, blobiness, B, C):
    noise, u64, _ = reference(P, blobiness, B)
    p1, p2 = patches(B, C, P)
    other = other_of(B)
    mask, _, out = run(noise, other, p1, p2, P, blobiness, 0.0)
    assert not mask.any() and torch.equal(bits(out), bits(p2))
    mask, field, out = run(noise, other, p1, p2, P, blobiness, 1.0)
    # all but the field's maximum
    top = field == 1.0
    assert torch.equal(mask != 0, ~top)
    for b in range(B):
        assert 1 <= int(top[b].sum()) <= 4 and field[b].flatten()[int(np.argmax(u64[b]))].item() >= 1.0 - BAND
    assert_composite(mask, other, p1, p2, out)


@pytest.mark.parametrize("P,blobiness,B,C", SHAPES)
def test_outputs_fully_written_and_repeatable(monkeypatch, P, blobiness, B, C):
    """mask, field and the scratch planes start NaN-filled between red zones (tests/poisoned_alloc.py): every output element is written,
    nothing outside is, the scratch needs no zeroing - and a second call gives the same bits."""
    import poisoned_alloc
    from bihome_amd import synth_gpu
    noise, _, _ = reference(P, blobiness, B)
    p1, p2 = patches(B, C, P)
    other = other_of(B)
    first = run(noise, other, p1, p2, P, blobiness, 0.3)
    pz = poisoned_alloc.poison(monkeypatch, synth_gpu)
    again = run(noise, other, p1, p2, P, blobiness, 0.3)
    assert pz.callers() == {"apply_blobs"}
    assert pz.verify() == (3 if P > 128 else 2)                       # mask, field (, scratch)
    for a, b in zip(first, again):
        assert not torch.isnan(b).any()
        assert torch.equal(bits(a), bits(b))
    assert_composite(again[0], other, p1, p2, again[2])


@pytest.mark.parametrize("P,C", [(32, 3), (128, 1), (256, 1)])
def test_constant_noise_is_no_blob(P, C):
    p1, p2 = patches(2, C, P)
    for value in (0.0, 0.7314):
        noise = np.full((2, P, P), value, np.float32)
        mask, field, out = run(noise, other_of(2), p1, p2, P, 0.2, 0.5)
        assert not mask.any() and not torch.isnan(field).any() and (field == 1).all()
        assert torch.equal(bits(out), bits(p2))


def test_bad_arguments_are_refused_without_a_launch():
    from bihome_amd import synth_gpu
    from bihome_amd._lib import BihomeLibError

    def call(B=2, C=1, P=32, sigma=1.6, porosity=0.3):
        z = torch.zeros(B, C, P, P, device="cuda")
        before = z.clone()
        with pytest.raises(BihomeLibError) as e:
            synth_gpu.apply_blobs(torch.zeros(B, P, P, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), z.clone(), z,
                                  sigma, porosity, want_field=True)
        torch.cuda.synchronize()
        assert torch.equal(z, before)
        return str(e.value)
    for kw in (dict(P=24), dict(P=272), dict(sigma=synth.blob_sigma(32, 0.05))):
        assert "BH_E_UNSUPPORTED" in call(**kw), kw
    for kw in (dict(B=1), dict(C=2), dict(porosity=1.5), dict(sigma=0.0)):
        assert "BH_E_BADARG" in call(**kw), kw
    with pytest.raises(ValueError):
        synth_gpu.apply_blobs(torch.zeros(2, 32, 32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                              torch.zeros(2, 1, 32, 32, device="cuda"), torch.zeros(2, 1, 16, 16, device="cuda"), 1.6, 0.3)


# ---- the generator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,md", [(1, 0), (3, 32)])
def test_generator_with_and_without_blobs(channels, md):
    from bihome_amd.synth_gpu import GpuPairGenerator
    kw = dict(n_images=3, seed=11, channels=channels, photometric_max_delta=md, photometric_draws="device")
    plain = GpuPairGenerator(**kw).next(4)
    d = GpuPairGenerator(blob_porosity=0.3, blobiness=0.5, **kw).next(4)
    assert set(d) == set(plain) | {"blob_mask", "blob_other"}
    assert torch.equal(bits(d["patch_1"]), bits(plain["patch_1"])) and torch.equal(d["delta"], plain["delta"])
    mask, other = d["blob_mask"], d["blob_other"]
    assert mask.shape == (4, 1, 128, 128) and mask.dtype == torch.float32 and other.shape == (4,)
    assert (other.cpu() != torch.arange(4)).all() and (other >= 0).all() and (other < 4).all()
    # patch_2 outside the mask is the plain generator's, inside it the other sample's patch_1: bit for bit
    assert_composite(mask[:, 0], other, plain["patch_1"], plain["patch_2"], d["patch_2"])
    assert 0.1 < mask.mean().item() < 0.5
    # the two extra draws come after all the others
    four, five = GpuPairGenerator(**kw).draw(4), GpuPairGenerator(blob_porosity=0.3, blobiness=0.5, **kw).draw(4)
    assert len(four) == 4 and len(five) == 5
    assert all(torch.equal(a, b) if a is not None else b is None for a, b in zip(four, five[:4]))
    noise, other = five[4]
    assert noise.shape == (4, 128, 128) and 0 <= noise.min() and noise.max() < 1 and other.dtype == torch.int32
    with pytest.raises(ValueError):
        GpuPairGenerator(blob_porosity=0.3, blobiness=0.5, **kw).next(1)


def test_from_config_batch_trains_one_step():
    from bihome_amd.step import build_loss, build_model, build_optimizer, train_step
    from bihome_amd.synth_gpu import GpuPairGenerator
    cfg = configs.get("zeng-bihome-pds-blobs")
    model = build_model(cfg)
    load_synthetic(model[0], 0)
    load_synthetic(model[1].auxiliary_resnet, 0)
    opt, sched = build_optimizer(model, cfg["SOLVER"])
    gen = GpuPairGenerator.from_config(cfg, n_images=2)
    assert gen.blobs and gen.blob_porosity == 0.1 and gen.blobiness == 0.2
    batch = gen.next(2)
    assert set(batch) == {"patch_1", "patch_2", "delta", "blob_mask", "blob_other"}
    assert batch["blob_mask"].shape == (2, 1, 128, 128) and 0.0 < batch["blob_mask"].mean().item() < 0.3
    assert batch["blob_other"].tolist() == [1, 0]
    loss, dgt, _ = train_step(model, dict(batch), opt, sched, loss_fn=build_loss(cfg["SOLVER"]))
    assert np.isfinite(loss.item())
    assert torch.equal(dgt.reshape(2, 4, 2), batch["delta"])


@pytest.mark.parametrize("C", [1, 3])
def test_fixture_through_the_kernel(golden, C):
    """The reference collator's own output (tests/golden/collator_blobs_b4.npz) from its recorded noise and indices."""
    g = golden("collator_blobs_b4")
    t = "c%d_" % C
    por, bl = float(g["porosity"]), float(g["blobiness"])
    u64 = np.stack([synth.blob_field(n.astype(np.float64), bl) for n in g[t + "noise"]])
    decided = np.abs(u64 - por) >= BAND
    assert 1.0 - decided.mean() <= 0.01
    p1, p2 = torch.tensor(g[t + "patch_1"]).cuda(), torch.tensor(g[t + "patch_2"]).cuda()
    other = torch.tensor(g[t + "other"], dtype=torch.int32).cuda()
    mask, _, out = run(g[t + "noise"], other, p1, p2, 32, bl, por)
    m = mask.cpu().numpy() != 0
    assert np.array_equal(m[decided], g[t + "mask"].astype(bool)[decided])
    d3 = np.broadcast_to(decided[:, None], g[t + "out"].shape)
    assert np.array_equal(out.cpu().numpy()[d3], g[t + "out"][d3])
    assert_composite(mask, other, p1, p2, out)
