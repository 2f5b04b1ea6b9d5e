"""Host side of the image bank (bihome_amd/bank.py, bh_bank_gather_u8), checked without a GPU: the sampler against a literal numpy
restatement of the reference's DatasetSampler (src/data/coco/dataset.py:106-157), `ImageBank.from_directory` on files written here,
the generator's bank-size rule, the header / ctypes agreement of the new entry point and its argument rules (every refusal returns
before a launch: without a device a call that got as far as a launch would return a hipError_t instead)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bihome_amd.bank import BankSampler, ImageBank
from bihome_amd.synth_gpu import GpuPairGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG = 0, -1


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
def _restated_epochs(rs, N, S, batch, epochs):
    """dataset.py:136-157 literally: one choice(np.arange(N), S) per epoch from a continuing state; a batch is yielded when its last
    sample arrives, so a trailing partial batch never is."""
    out = []
    for _ in range(epochs):
        order = rs.choice(np.arange(N), S)
        batches, cur = [], []
        for i, k in enumerate(order):
            cur.append(k)
            if i % batch == batch - 1:
                batches.append(np.array(cur))
                cur = []
        out.append(batches)
    return out


def test_sampler_is_the_reference_order_over_two_epochs():
    N, batch, S, seed = 7, 4, 10, 123
    s = BankSampler(N, batch, S, seed=seed)
    assert len(s) == 2
    got = [list(s), list(s)]
    want = _restated_epochs(np.random.RandomState(seed), N, S, batch, 2)
    for g, w in zip(got, want):
        assert len(g) == len(w) == 2
        for a, b in zip(g, w):
            assert a.shape == (batch,) and np.array_equal(a, b)
    assert not np.array_equal(np.concatenate(got[0]), np.concatenate(got[1]))        # the state continues: a new epoch, a new order
    assert all(0 <= k < N for e in got for b in e for k in b)
    # a second sampler with the same seed starts over
    assert np.array_equal(np.concatenate(list(BankSampler(N, batch, S, seed=seed))), np.concatenate(got[0]))


def test_sampler_without_a_seed_draws_from_the_global_state():
    N, batch, S = 7, 4, 10
    np.random.seed(5)
    s = BankSampler(N, batch, S)
    got = [list(s), list(s)]
    np.random.seed(5)
    want = _restated_epochs(np.random, N, S, batch, 2)
    for g, w in zip(got, want):
        assert len(g) == len(w) == len(s) == 2
        for a, b in zip(g, w):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------
# ImageBank
# ------------------------------------------------------------------------------------------------
def _save(tmp_path, names, shape=(6, 8, 3), seed=0):
    rs = np.random.RandomState(seed)
    arrays = {}
    for n in names:
        arrays[n] = rs.randint(0, 256, shape).astype(np.uint8)
        np.save(tmp_path / n, arrays[n])
    return arrays


def test_from_directory_loads_in_sorted_order(tmp_path):
    names = ["b.npy", "a.npy", "c10.npy", "c9.npy", "0.npy"]                  # (written in this order)
    arrays = _save(tmp_path, names)
    (tmp_path / "notes.txt").write_text("not an image")
    bank = ImageBank.from_directory(str(tmp_path), device="cpu")
    assert len(bank) == 5 and (bank.h, bank.w) == (6, 8) and bank.nbytes == 5 * 6 * 8 * 3
    assert bank.data.dtype == torch.uint8 and bank.data.is_contiguous() and tuple(bank.data.shape) == (5, 6, 8, 3)
    for k, n in enumerate(sorted(names)):
        assert np.array_equal(bank.data[k].numpy(), arrays[n]), n
    first = ImageBank.from_directory(str(tmp_path), max_images=2, device="cpu")
    assert len(first) == 2 and torch.equal(first.data, bank.data[:2])


def test_from_directory_uploads_in_chunks(tmp_path, monkeypatch):
    from bihome_amd import bank as bank_module
    arrays = _save(tmp_path, ["%02d.npy" % i for i in range(7)])
    monkeypatch.setattr(bank_module, "UPLOAD_CHUNK_BYTES", 3 * 6 * 8 * 3)            # three images per upload: 3 + 3 + 1
    bank = ImageBank.from_directory(str(tmp_path), device="cpu")
    assert np.array_equal(bank.data.numpy(), np.stack([arrays["%02d.npy" % i] for i in range(7)]))


@pytest.mark.parametrize("name,array", [
    ("bad_f64.npy", np.zeros((6, 8, 3), np.float64)),
    ("bad_gray.npy", np.zeros((6, 8), np.uint8)),
    ("bad_rgba.npy", np.zeros((6, 8, 4), np.uint8)),
    ("bad_size.npy", np.zeros((6, 9, 3), np.uint8)),
])
def test_from_directory_names_the_offending_file(tmp_path, name, array):
    _save(tmp_path, ["a.npy", "b.npy"])
    np.save(tmp_path / name, array)                                          # ("bad_..." sorts after a and b)
    with pytest.raises(ValueError, match=re.escape(name)):
        ImageBank.from_directory(str(tmp_path), device="cpu")


def test_from_directory_refuses_jpeg(tmp_path):
    _save(tmp_path, ["a.npy"])
    (tmp_path / "COCO_train2014_000000000009.jpg").write_bytes(b"\xff\xd8\xff")
    with pytest.raises(ValueError, match=r"COCO_train2014_000000000009\.jpg.*decoder.*preprocess_offline\.py"):
        ImageBank.from_directory(str(tmp_path), device="cpu")


def test_image_bank_refuses_other_layouts_before_any_device_work():
    # (device="cuda" is never reached: the checks come first)
    for bad in (np.zeros((2, 6, 8, 3), np.float32), np.zeros((6, 8, 3), np.uint8), np.zeros((2, 6, 8, 4), np.uint8),
                np.zeros((0, 6, 8, 3), np.uint8), torch.zeros(2, 3, 6, 8, dtype=torch.uint8), torch.zeros(2, 6, 8, 3)):
        with pytest.raises(ValueError):
            ImageBank(bad, device="cuda")
    bank = ImageBank(np.arange(2 * 6 * 8 * 3, dtype=np.uint8).reshape(2, 6, 8, 3), device="cpu")
    assert len(bank) == 2 and (bank.h, bank.w, bank.nbytes) == (6, 8, 288)


def test_generator_refuses_a_bank_smaller_than_the_patch_and_its_margin():
    kw = dict(patch=32, rho=4, device="cpu")
    with pytest.raises(ValueError, match="40"):
        GpuPairGenerator(bank=ImageBank(np.zeros((1, 39, 52, 3), np.uint8), device="cpu"), **kw)
    with pytest.raises(ValueError):
        GpuPairGenerator(bank=ImageBank(np.zeros((1, 52, 39, 3), np.uint8), device="cpu"), **kw)
    gen = GpuPairGenerator(bank=ImageBank(np.zeros((3, 40, 40, 3), np.uint8), device="cpu"), **kw)
    assert (gen.h, gen.w, gen.n_images) == (40, 40, 3)
    # the only position left (transforms.py:505-506), whatever the seed; a host index outside the bank is refused before any launch
    idx, origin, _, _ = gen.draw(5, idx=[0, 2, 1, 2, 0])
    assert idx.tolist() == [0, 2, 1, 2, 0] and idx.dtype == torch.int32 and (origin == 4).all()
    for bad in ([0, 1, 3, 0, 0], [0, -1, 0, 0, 0], [0, 1], [0.0, 1.0, 2.0, 0.0, 1.0]):
        with pytest.raises(ValueError):
            gen.draw(5, idx=bad)


def test_an_index_given_to_draw_leaves_every_other_draw_alone():
    bank = ImageBank(np.zeros((3, 60, 70, 3), np.uint8), device="cpu")
    kw = dict(patch=32, rho=8, seed=9, photometric_max_delta=32, photometric_draws="device", blob_porosity=0.3, blobiness=0.5,
              device="cpu", bank=bank)
    own, given = GpuPairGenerator(**kw).draw(4), GpuPairGenerator(**kw).draw(4, idx=np.array([2, 2, 0, 1]))
    assert given[0].tolist() == [2, 2, 0, 1]
    for a, b in zip(own[1:4], given[1:4]):
        assert torch.equal(a, b)
    assert torch.equal(own[4][0], given[4][0]) and torch.equal(own[4][1], given[4][1])


# ------------------------------------------------------------------------------------------------
# the C entry point
# ------------------------------------------------------------------------------------------------
def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bh_bank_gather_u8\s*\(([^)]*)\)\s*;", text)
    assert m, "include/bihome.h does not declare bh_bank_gather_u8"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const unsigned char* bank", "const int* img_idx", "int count", "int n_images", "int Hs", "int Ws", "float* out",
                    "void* stream"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["bh_bank_gather_u8"] == [P, P, I, I, I, I, P, P]
    assert list(_lib.lib.bh_bank_gather_u8.argtypes) == [P, P, I, I, I, I, P, P] and _lib.lib.bh_bank_gather_u8.restype is I
    # the header says what an index outside the bank does, and cites what the entry point replaces
    raw = " ".join(open(os.path.join(ROOT, "include", "bihome.h")).read().split())
    doc = raw[:raw.index("int bh_bank_gather_u8(")].rsplit("/*", 1)[1]
    assert "CLAMPED" in doc and "src/data/coco/dataset.py:95-103" in doc


def test_c_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_bank_gather_u8, ctypes.c_void_p(64)

    def call(bank=p, img_idx=p, count=2, n_images=5, Hs=24, Ws=32, out=p):
        return f(bank, img_idx, count, n_images, Hs, Ws, out, None)
    for bad in (dict(bank=None), dict(img_idx=None), dict(out=None), dict(count=-1), dict(n_images=0), dict(n_images=-3), dict(Hs=0),
                dict(Hs=-1), dict(Ws=0), dict(Ws=-1), dict(count=0, out=None), dict(count=0, Ws=0)):
        assert call(**bad) == BH_E_BADARG, bad
    for ok in (dict(count=0), dict(count=0, Hs=23, Ws=37), dict(count=0, n_images=1, Hs=1, Ws=1)):
        assert call(**ok) == BH_OK, ok                                       # an empty batch: nothing launched
    if not torch.cuda.is_available():
        assert call() > 0                                                    # (an accepted call does launch: the launch's own error)
