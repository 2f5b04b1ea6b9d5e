"""Raw-size images into the image bank on the device (bh_bank_ingest_u8, csrc/bank.hip; ImageBank.from_images / from_directory with
size=).  Every comparison is bitwise against bihome_amd.bank.rescale_center_crop_host, the numpy statement of upstream's Rescale +
CenterCrop (tests/test_bank_ingest_cpu.py holds that to upstream's sizes and to a float64 resample)."""
import functools

import numpy as np
import pytest
import torch

import poisoned_alloc
from bihome_amd.bank import rescale_center_crop_host, rescale_size

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# target (W, H) = (8, 6): exact halving; copy; landscape (crop in x); portrait (crop in y); upscale (both edge clamps); a single column;
# a single row; halving in x only (nh = round(6.5) = 6: the fixed-point path)
RAGGED = [(12, 16), (6, 8), (11, 17), (19, 9), (5, 7), (3, 1), (1, 3), (13, 16)]


@functools.lru_cache(maxsize=None)
def image(h, w, seed=0):
    """uint8 [h,w,3] random, made once per shape and shared; callers do not modify it."""
    a = np.random.RandomState(seed + 1000 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host(h, w, size, seed=0):
    out = rescale_center_crop_host(image(h, w, seed), size)
    out.setflags(write=False)
    return out


def pack(arrays, gap=0):
    """(src on the device, src_off, src_hw on the host): the images back to back, `gap` unused bytes in front of each."""
    off, parts, at = [], [], 0
    for a in arrays:
        parts.append(np.full(gap, SENTINEL, np.uint8))
        off.append(at + gap)
        parts.append(np.asarray(a).reshape(-1))
        at += gap + a.nbytes
    return (torch.from_numpy(np.concatenate(parts)).cuda(), np.asarray(off, np.int64),
            np.asarray([a.shape[:2] for a in arrays], np.int32).reshape(-1, 2))


def test_the_ragged_sizes_cover_the_three_paths():
    kinds = []
    for h, w in RAGGED:
        nh, nw, top, left = rescale_size(h, w, (8, 6))
        kinds.append("halve" if (h, w) == (2 * nh, 2 * nw) else "copy" if (h, w) == (nh, nw) else "fixed")
    assert kinds == ["halve", "copy", "fixed", "fixed", "fixed", "fixed", "fixed", "fixed"]
    assert rescale_size(11, 17, (8, 6)) == (6, 9, 0, 0) and rescale_size(19, 9, (8, 6)) == (17, 8, 5, 0)      # 8 of 9 columns, 6 of 17 rows
    assert rescale_size(5, 7, (8, 6)) == (6, 8, 0, 0) and rescale_size(13, 16, (8, 6)) == (6, 8, 0, 0)
    assert rescale_size(11, 17, (7, 6)) == (6, 9, 0, 1)                                                      # W = 7: a crop from column 1


@pytest.mark.parametrize("W,odd_base", [(8, False), (7, False), (8, True), (7, True)],
                         ids=["W8-dword-stores", "W7-byte-stores", "W8-odd-base-byte-stores", "W7-odd-base"])
def test_one_ragged_launch_fills_its_slots_and_nothing_else(W, odd_base):
    """first = 2 in a bank of n + 4 slots pre-filled with a sentinel, between red zones; launched twice: the same bytes."""
    from bihome_amd import kernels as K
    H, n = 6, len(RAGGED)
    arrays = [image(h, w) for h, w in RAGGED]
    want = np.stack([host(h, w, (W, H)) for h, w in RAGGED])
    src, off, hw = pack(arrays, gap=1)                                   # (gap 1: every image starts on another byte alignment)
    p = poisoned_alloc.Poisoned()
    nbytes = (n + 4) * H * W * 3
    raw = p.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
    raw.fill_(SENTINEL)
    bank = raw[1:1 + nbytes].view(n + 4, H, W, 3) if odd_base else raw[:nbytes].view(n + 4, H, W, 3)
    assert bank.data_ptr() % 4 == (1 if odd_base else 0) and bank.is_contiguous()
    assert K.bank_ingest_u8(src, off, hw, bank, first=2) is bank
    got = bank.cpu().numpy()
    for k, (h, w) in enumerate(RAGGED):
        assert np.array_equal(got[2 + k], want[k]), "source %d x %d -> %d x %d" % (h, w, H, W)
    assert (got[:2] == SENTINEL).all() and (got[2 + n:] == SENTINEL).all()
    outside = raw.cpu().numpy()
    assert (outside[:1 if odd_base else 0] == SENTINEL).all() and (outside[(1 if odd_base else 0) + nbytes:] == SENTINEL).all()
    assert p.verify() == 1                                               # the red zones before and after the allocation
    again = torch.full_like(bank, SENTINEL)
    K.bank_ingest_u8(src, off, hw, again, first=2)
    assert torch.equal(again, bank)


def test_value_regimes():
    """all 0, all 255, a 0 / 255 checkerboard and random bytes through the fixed-point path ((11, 17) -> (8, 6)) and the halving path."""
    from bihome_amd import kernels as K
    arrays = []
    for h, w in ((11, 17), (12, 16)):
        board = np.broadcast_to((((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2) * 255).astype(np.uint8)[:, :, None], (h, w, 3))
        arrays += [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), np.ascontiguousarray(board), image(h, w, seed=3)]
    src, off, hw = pack(arrays)
    bank = torch.full((len(arrays), 6, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    K.bank_ingest_u8(src, off, hw, bank)
    got = bank.cpu().numpy()
    for k, a in enumerate(arrays):
        assert np.array_equal(got[k], rescale_center_crop_host(a, (8, 6))), k
    assert (got[0] == 0).all() and (got[1] == 255).all() and (got[4] == 0).all() and (got[5] == 255).all()
    assert set(np.unique(got[6])) == {127 + 1}                           # 2x2 blocks of a checkerboard: (0 + 255 + 255 + 0 + 2) >> 2


def test_offsets_are_64_bit_on_both_sides():
    """A bank of 4 x 6-pixel slots (72 bytes) whose total passes 2^31 bytes, two images into slots that start past 2^31; the same two
    images read from offsets past 2^31 of an uninitialised source buffer."""
    from bihome_amd import kernels as K
    W, H, slot = 4, 6, 72
    first = 2 ** 31 // slot + 2                                          # slot 29,826,163 starts at byte 2,147,483,736
    n_slots = first + 8
    assert (first - 1) * slot > 2 ** 31 and n_slots * slot < 2 ** 32
    bank = torch.empty((n_slots, H, W, 3), dtype=torch.uint8, device="cuda")
    bank[first - 1:first + 3] = SENTINEL
    arrays = [image(12, 8), image(11, 17)]                               # halving and fixed-point
    want = [host(12, 8, (W, H)), host(11, 17, (W, H))]
    src = torch.empty(2 ** 31 + 4096, dtype=torch.uint8, device="cuda")
    off = np.asarray([2 ** 31 + 5, 2 ** 31 + 5 + arrays[0].nbytes + 2], np.int64)
    for o, a in zip(off, arrays):
        src[int(o):int(o) + a.nbytes] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    K.bank_ingest_u8(src, off, np.asarray([a.shape[:2] for a in arrays], np.int32), bank, first=first)
    got = bank[first - 1:first + 3].cpu().numpy()
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])
    assert (got[0] == SENTINEL).all() and (got[3] == SENTINEL).all()     # the slot before and the slot after


def test_wrapper_checks_the_host_tables_before_upload():
    from bihome_amd import kernels as K
    src, off, hw = pack([image(6, 8), image(5, 7)])
    bank = torch.full((3, 6, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    for bad_hw in ([[6, 8], [0, 7]], [[6, 8], [5, 0]], [[6, 8], [-5, 7]], [[6, 8], [5, 8]]):          # (5 x 8 ends past src)
        with pytest.raises(ValueError):
            K.bank_ingest_u8(src, off, np.asarray(bad_hw, np.int32), bank)
    for bad_off in ([-1, 144], [0, 145]):
        with pytest.raises(ValueError):
            K.bank_ingest_u8(src, np.asarray(bad_off, np.int64), hw, bank)
    for first in (-1, 2):
        with pytest.raises(ValueError):
            K.bank_ingest_u8(src, off, hw, bank, first=first)
    with pytest.raises(ValueError):
        K.bank_ingest_u8(src, off.astype(np.int32), hw, bank)
    assert (bank == SENTINEL).all()
    # on the device the tables cannot be checked: an image without pixels leaves its slot untouched (include/bihome.h)
    K.bank_ingest_u8(src, torch.from_numpy(off).cuda(), torch.tensor([[6, 8], [0, 7]], dtype=torch.int32, device="cuda"), bank, first=1)
    got = bank.cpu().numpy()
    assert (got[0] == SENTINEL).all() and np.array_equal(got[1], image(6, 8)) and (got[2] == SENTINEL).all()


def test_from_directory_with_size_end_to_end(tmp_path, monkeypatch):
    """Five mixed-size files through from_directory(size=(80, 64)) on the device with a forced chunk boundary: the CPU bank's bytes, and
    a generator on it returns what a generator on a bank built directly from the host-resized array returns."""
    from bihome_amd import bank as bank_module
    from bihome_amd.bank import BankSampler, ImageBank
    from bihome_amd.synth_gpu import GpuPairGenerator
    sizes = [(128, 160), (64, 80), (100, 150), (150, 90), (50, 60)]     # halving, copy, crop in x, crop in y, upscale
    for k, (h, w) in enumerate(sizes):
        np.save(tmp_path / ("%d.npy" % k), image(h, w, seed=k))
    monkeypatch.setattr(bank_module, "UPLOAD_CHUNK_BYTES", 128 * 160 * 3 + 64 * 80 * 3)      # chunks of 2, 1 (150 x 90 does not fit), 2 images
    bank = ImageBank.from_directory(str(tmp_path), size=(80, 64))
    assert bank.data.is_cuda and tuple(bank.data.shape) == (5, 64, 80, 3)
    on_cpu = ImageBank.from_directory(str(tmp_path), size=(80, 64), device="cpu")
    want = np.stack([rescale_center_crop_host(image(h, w, seed=k), (80, 64)) for k, (h, w) in enumerate(sizes)])
    assert np.array_equal(on_cpu.data.numpy(), want) and np.array_equal(bank.data.cpu().numpy(), want)
    assert torch.equal(ImageBank.from_images([image(h, w, seed=k) for k, (h, w) in enumerate(sizes)], (80, 64)).data, bank.data)
    gen = GpuPairGenerator(patch=32, rho=8, seed=5, bank=bank)
    twin = GpuPairGenerator(patch=32, rho=8, seed=5, bank=ImageBank(want))
    a, b = gen.next(4, idx=[4, 0, 2, 2]), twin.next(4, idx=[4, 0, 2, 2])
    assert set(a) == set(b) and a["patch_1"].shape == (4, 1, 32, 32)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ea = list(gen.epoch(BankSampler(len(bank), 4, 9, seed=2)))
    eb = list(twin.epoch(BankSampler(len(bank), 4, 9, seed=2)))
    assert len(ea) == len(eb) == 2
    for x, y in zip(ea, eb):
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_ingest_is_capturable():
    """One ingest under torch.cuda.graph (tables already on the device: nothing is copied), replayed once: the eager bytes."""
    from bihome_amd import kernels as K
    arrays = [image(h, w) for h, w in RAGGED]
    src, off, hw = pack(arrays)
    off, hw = torch.from_numpy(off).cuda(), torch.from_numpy(hw).cuda()
    eager = torch.full((len(arrays) + 2, 6, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.bank_ingest_u8(src, off, hw, eager, first=1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static = torch.full_like(eager, SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.bank_ingest_u8(src, off, hw, static, first=1)
    static.fill_(SENTINEL)                                               # (the capture recorded the launch, it did not run it)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    assert np.array_equal(eager.cpu().numpy()[1:-1], np.stack([host(h, w, (8, 6)) for h, w in RAGGED]))
