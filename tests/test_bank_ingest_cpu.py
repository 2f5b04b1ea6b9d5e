"""Raw-size images into the image bank, checked without a GPU (bihome_amd/bank.py: rescale_size, rescale_center_crop_host,
ImageBank.from_images, ImageBank.from_directory with size=; the C entry point bh_bank_ingest_u8 as far as it goes without a device).

`rescale_center_crop_host` is upstream's Rescale + CenterCrop (src/data/transforms.py:24-46, 103-122) with cv2.resize's INTER_LINEAR on
8-bit data as recalled: it is the reference the kernel is held to bit for bit (tests/test_bank_ingest_gpu.py), so here it is held to
what can be known without cv2: upstream's sizes worked out by hand, the properties of its three paths, and an independent float64
bilinear resample."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

from bihome_amd import bank as bank_module
from bihome_amd.bank import ImageBank, rescale_center_crop_host, rescale_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH_OK, BH_E_BADARG = 0, -1


@functools.lru_cache(maxsize=None)
def image(h, w, seed=0):
    """uint8 [h,w,3] random, made once per shape and shared; callers do not modify it."""
    a = np.random.RandomState(seed + 1000 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------
# rescale_size
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,size,want", [
    ((480, 640), (320, 240), (240, 320, 0, 0)),         # r = 0.75 = H / W: not below it, nh = round(320 * 0.75)
    ((427, 640), (320, 240), (240, 360, 0, 20)),        # r = 0.6672 < 0.75: nw = round(240 / 0.66719) = round(359.72)
    ((640, 480), (320, 240), (427, 320, 93, 0)),        # r = 1.3333: nh = round(426.67), top = 187 // 2
    ((240, 320), (320, 240), (240, 320, 0, 0)),         # identity
    ((32, 32), (192, 192), (192, 192, 0, 0)),           # CIFAR: an upscale
    ((5, 4), (2, 1), (2, 2, 0, 0)),                     # W r = 2.5 exactly: numpy rounds half to EVEN, 2 (half up would be 3)
    ((7, 4), (2, 1), (4, 2, 1, 0)),                     # W r = 3.5 exactly: 4, top = 3 // 2
    ((512, 640), (320, 256), (256, 320, 0, 0)),         # FLIR ADAS: r = 0.8 = H / W in double as well
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_rescale_size_is_upstreams(hw, size, want):
    assert rescale_size(hw[0], hw[1], size) == want
    assert all(type(v) is int for v in rescale_size(hw[0], hw[1], size))


def test_rescale_size_refusals():
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            rescale_size(bad[0], bad[1], (8, 6))
    for bad in ((0, 6), (8, 0), (8,), (8, 6, 3), 8, (8.5, 6), None):
        with pytest.raises(ValueError):
            rescale_size(4, 4, bad)


# ------------------------------------------------------------------------------------------------
# the host statement: properties of the three paths
# ------------------------------------------------------------------------------------------------
SOURCES = [(12, 16), (6, 8), (11, 17), (19, 9), (5, 7), (3, 1), (1, 3), (13, 16)]        # -> (W, H) = (8, 6): halving, copy, fixed-point...


def test_exact_halving_is_the_rounded_2x2_mean():
    a = image(12, 16)
    assert rescale_size(12, 16, (8, 6)) == (6, 8, 0, 0)
    s = a.astype(np.int64)
    want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) // 4
    assert np.array_equal(rescale_center_crop_host(a, (8, 6)), want)
    # halving with a crop: 12 x 20 -> 6 x 10, columns 1 .. 8 of it
    b = image(12, 20)
    assert rescale_size(12, 20, (8, 6)) == (6, 10, 0, 1)
    s = b.astype(np.int64)
    want = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) // 4)[:, 1:9]
    assert np.array_equal(rescale_center_crop_host(b, (8, 6)), want)
    # halving in x only is NOT this path: 13 x 16 -> 6 x 8 (nh = round(6.5) = 6)
    assert rescale_size(13, 16, (8, 6)) == (6, 8, 0, 0)


def test_same_size_is_a_copy():
    a = image(6, 8)
    out = rescale_center_crop_host(a, (8, 6))
    assert np.array_equal(out, a) and out is not a and out.flags.c_contiguous
    # the same size after Rescale, then a crop: 6 x 8 with target (4, 6) keeps nh = 6, nw = round(6 / 0.75) = 8
    assert rescale_size(6, 8, (4, 6)) == (6, 8, 0, 2)
    assert np.array_equal(rescale_center_crop_host(a, (4, 6)), a[:, 2:6])


@pytest.mark.parametrize("value", [0, 1, 127, 255])
def test_a_constant_image_stays_that_constant(value):
    for h, w in SOURCES + [(12, 20), (640, 480)]:
        out = rescale_center_crop_host(np.full((h, w, 3), value, np.uint8), (8, 6))
        assert out.shape == (6, 8, 3) and out.dtype == np.uint8 and (out == value).all(), (h, w, np.unique(out))


def test_output_shape_is_always_h_w_3():
    for h, w in SOURCES:
        for size in ((8, 6), (7, 6), (1, 1), (5, 9), (192, 192)):
            out = rescale_center_crop_host(image(h, w), size)
            assert out.shape == (size[1], size[0], 3) and out.dtype == np.uint8 and out.flags.c_contiguous, (h, w, size)


def test_host_statement_refusals():
    for bad in (np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.uint8), np.zeros((6, 8, 4), np.uint8), np.zeros((0, 8, 3), np.uint8),
                np.zeros((6, 0, 3), np.uint8)):
        with pytest.raises(ValueError):
            rescale_center_crop_host(bad, (8, 6))
    with pytest.raises(ValueError):
        rescale_center_crop_host(image(6, 8), (0, 6))


# ------------------------------------------------------------------------------------------------
# the host statement against an independent float64 bilinear resample
# ------------------------------------------------------------------------------------------------
def bilinear_float64(img, size):
    """The cropped window of `img` resampled to the Rescale size with half-pixel centres and edge clamp, in float64, unrounded."""
    (W, H), (h, w) = size, img.shape[:2]
    nh, nw, top, left = rescale_size(h, w, size)

    def axis(n, n_new, first, count):
        p = (np.arange(count) + first + 0.5) * n / n_new - 0.5
        i = np.floor(p)
        return np.clip(i, 0, n - 1).astype(int), np.clip(i + 1, 0, n - 1).astype(int), p - i
    y0, y1, fy = axis(h, nh, top, H)
    x0, x1, fx = axis(w, nw, left, W)
    s, fy, fx = img.astype(np.float64), fy[:, None, None], fx[None, :, None]
    return (s[y0][:, x0] * (1 - fx) + s[y0][:, x1] * fx) * (1 - fy) + (s[y1][:, x0] * (1 - fx) + s[y1][:, x1] * fx) * fy


@pytest.mark.parametrize("h,w", [(11, 17), (19, 9), (5, 7), (3, 1), (1, 3)])
def test_fixed_point_path_against_float64_bilinear(h, w):
    """The bound is DERIVED: coefficient rounding at most 255 / 4096 per tap pair per axis, the >> 4 under 0.01, the two >> 16
    truncations at most 0.25 each, the final rounding 0.5 - about 1.3 in all, so the distance of an integer output from the unrounded
    float64 value is below 2.  On these inputs (20 random images per size) the largest distance seen on the CPU is 0.76, so the bound
    asserted here is the tighter 1."""
    nh, nw, _, _ = rescale_size(h, w, (8, 6))
    assert (nh, nw) != (h, w) and not (h == 2 * nh and w == 2 * nw)                   # the fixed-point path
    worst = 0.0
    for seed in range(20):
        a = image(h, w, seed)
        worst = max(worst, np.abs(rescale_center_crop_host(a, (8, 6)).astype(np.float64) - bilinear_float64(a, (8, 6))).max())
    print("(%d, %d) -> (8, 6): max |host - float64 bilinear| = %.4f" % (h, w, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------
# ImageBank.from_images / from_directory(size=) on the CPU
# ------------------------------------------------------------------------------------------------
def host_bank(arrays, size):
    return np.stack([rescale_center_crop_host(a, size) for a in arrays])


def test_from_images_equals_the_host_statement():
    arrays = [image(h, w) for h, w in SOURCES]
    bank = ImageBank.from_images(arrays, (8, 6), device="cpu")
    assert len(bank) == len(SOURCES) and (bank.h, bank.w) == (6, 8) and bank.data.dtype == torch.uint8 and bank.data.is_contiguous()
    assert np.array_equal(bank.data.numpy(), host_bank(arrays, (8, 6)))
    assert np.array_equal(ImageBank.from_images(arrays[:3], (7, 5), device="cpu").data.numpy(), host_bank(arrays[:3], (7, 5)))


def test_from_images_refusals():
    ok = image(6, 8)
    for bad in (np.zeros((6, 8, 3), np.float32), np.zeros((6, 8, 4), np.uint8), np.zeros((6, 8), np.uint8), np.zeros((0, 8, 3), np.uint8),
                np.zeros((6, 0, 3), np.uint8)):
        with pytest.raises(ValueError, match="image 1"):
            ImageBank.from_images([ok, bad], (8, 6), device="cpu")
    for size in ((0, 6), (8, 0), (-1, 6), (8,)):
        with pytest.raises(ValueError):
            ImageBank.from_images([ok], size, device="cpu")
    with pytest.raises(ValueError):
        ImageBank.from_images([], (8, 6), device="cpu")
    # (device="cuda" is never reached: the checks come first)
    with pytest.raises(ValueError):
        ImageBank.from_images([ok, np.zeros((6, 8, 3), np.int8)], (8, 6), device="cuda")


def save_mixed(tmp_path, names, sizes=SOURCES):
    arrays = {}
    for k, n in enumerate(names):
        h, w = sizes[k % len(sizes)]
        arrays[n] = image(h, w, seed=k)
        np.save(tmp_path / n, arrays[n])
    return arrays


def test_from_directory_with_size_takes_mixed_sizes_in_sorted_order(tmp_path):
    names = ["b.npy", "a.npy", "c10.npy", "c9.npy", "0.npy", "d.npy", "e.npy", "f.npy"]          # (written in this order)
    arrays = save_mixed(tmp_path, names)
    (tmp_path / "notes.txt").write_text("not an image")
    bank = ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))
    assert tuple(bank.data.shape) == (8, 6, 8, 3) and bank.data.dtype == torch.uint8
    assert np.array_equal(bank.data.numpy(), host_bank([arrays[n] for n in sorted(names)], (8, 6)))
    first = ImageBank.from_directory(str(tmp_path), max_images=3, device="cpu", size=(8, 6))
    assert len(first) == 3 and torch.equal(first.data, bank.data[:3])


@pytest.mark.parametrize("chunk", [1, 200, 12 * 16 * 3, 12 * 16 * 3 + 6 * 8 * 3, 1 << 20])
def test_from_directory_with_size_packs_chunks(tmp_path, monkeypatch, chunk):
    """Chunks of 1 byte (every image larger than a chunk), 200 bytes (6 x 8 fits, 12 x 16 = 576 bytes travels alone), exactly one or two
    images, and everything in one."""
    names = ["%02d.npy" % i for i in range(9)]
    arrays = save_mixed(tmp_path, names)
    monkeypatch.setattr(bank_module, "UPLOAD_CHUNK_BYTES", chunk)
    bank = ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))
    assert np.array_equal(bank.data.numpy(), host_bank([arrays[n] for n in names], (8, 6)))
    assert np.array_equal(ImageBank.from_images([arrays[n] for n in names], (8, 6), device="cpu").data.numpy(), bank.data.numpy())


@pytest.mark.parametrize("name,array", [
    ("bad_f64.npy", np.zeros((6, 8, 3), np.float64)),
    ("bad_gray.npy", np.zeros((6, 8), np.uint8)),
    ("bad_rgba.npy", np.zeros((6, 8, 4), np.uint8)),
    ("bad_empty.npy", np.zeros((0, 8, 3), np.uint8)),
])
def test_from_directory_with_size_names_the_offending_file(tmp_path, name, array):
    save_mixed(tmp_path, ["a.npy", "b.npy"])
    np.save(tmp_path / name, array)                                          # ("bad_..." sorts after a and b)
    with pytest.raises(ValueError, match=re.escape(name)):
        ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))


def test_from_directory_with_size_decodes_png_exactly(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    arrays = save_mixed(tmp_path, ["a.npy", "c.npy"])
    png = image(11, 17, seed=7)
    Image.fromarray(np.asarray(png)).save(tmp_path / "b.PNG")                # (a mixed directory; the suffix in capitals)
    bank = ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))
    assert np.array_equal(bank.data.numpy(), host_bank([arrays["a.npy"], png, arrays["c.npy"]], (8, 6)))


def test_from_directory_with_size_takes_jpeg_as_pil_decodes_it(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    smooth = np.clip(np.add.outer(np.arange(40) * 5, np.arange(56) * 3)[:, :, None] + np.array([0, 20, 40]), 0, 255).astype(np.uint8)
    Image.fromarray(smooth).save(tmp_path / "x.jpg", quality=90)
    Image.fromarray(smooth[:32]).save(tmp_path / "y.jpeg", quality=90)
    with Image.open(tmp_path / "x.jpg") as im:
        x = np.asarray(im.convert("RGB"))
    with Image.open(tmp_path / "y.jpeg") as im:
        y = np.asarray(im.convert("RGB"))
    assert x.shape == (40, 56, 3) and y.shape == (32, 56, 3)
    bank = ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))
    assert np.array_equal(bank.data.numpy(), host_bank([x, y], (8, 6)))


def test_without_pil_the_first_image_file_is_named(tmp_path, monkeypatch):
    save_mixed(tmp_path, ["a.npy"])
    (tmp_path / "m.png").write_bytes(b"\x89PNG")
    (tmp_path / "k.jpg").write_bytes(b"\xff\xd8\xff")
    monkeypatch.setitem(sys.modules, "PIL", None)                            # `import PIL` now raises ImportError
    with pytest.raises(ValueError, match=r"k\.jpg.*no decoder is available"):
        ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))
    # ... and .npy files alone need no decoder
    os.remove(tmp_path / "m.png")
    os.remove(tmp_path / "k.jpg")
    assert len(ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))) == 1


def test_an_undecodable_image_file_is_named(tmp_path):
    pytest.importorskip("PIL.Image")
    save_mixed(tmp_path, ["a.npy"])
    (tmp_path / "broken.jpg").write_bytes(b"\xff\xd8\xff")
    with pytest.raises(ValueError, match=r"broken\.jpg"):
        ImageBank.from_directory(str(tmp_path), device="cpu", size=(8, 6))


def test_without_size_nothing_changes(tmp_path):
    save_mixed(tmp_path, ["a.npy", "b.npy"], sizes=[(6, 8), (6, 9)])
    with pytest.raises(ValueError, match=r"b\.npy.*one bank holds one size"):
        ImageBank.from_directory(str(tmp_path), device="cpu")
    os.remove(tmp_path / "b.npy")
    (tmp_path / "c.jpg").write_bytes(b"\xff\xd8\xff")
    with pytest.raises(ValueError, match=r"c\.jpg.*decoder.*preprocess_offline\.py"):
        ImageBank.from_directory(str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match=r"c\.jpg.*decoder.*preprocess_offline\.py"):
        ImageBank.from_directory(str(tmp_path), device="cpu", size=None)
    with pytest.raises(ValueError, match="no .npy"):
        ImageBank.from_directory(str(tmp_path), max_images=0, device="cpu", size=(8, 6))


def test_kernel_wrapper_checks_the_host_tables_before_any_device_work():
    """K.bank_ingest_u8: CPU tensors are refused as everywhere; the table checks themselves need device tensors and are in the GPU file."""
    from bihome_amd import kernels as K
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.bank_ingest_u8(torch.zeros(144, dtype=torch.uint8), np.zeros(1, np.int64), np.array([[6, 8]], np.int32),
                         torch.zeros(1, 6, 8, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------
# the C entry point
# ------------------------------------------------------------------------------------------------
def test_header_declares_what_ctypes_binds():
    from bihome_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bihome.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bh_bank_ingest_u8\s*\(([^)]*)\)\s*;", text)
    assert m, "include/bihome.h does not declare bh_bank_ingest_u8"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const unsigned char* src", "const int64_t* src_off", "const int* src_hw", "int count", "unsigned char* bank",
                    "int n_slots", "int first", "int H", "int W", "void* stream"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["bh_bank_ingest_u8"] == [P, P, P, I, P, I, I, I, I, P]
    assert list(_lib.lib.bh_bank_ingest_u8.argtypes) == [P, P, P, I, P, I, I, I, I, P] and _lib.lib.bh_bank_ingest_u8.restype is I
    # the header cites what the entry point replaces, says what a bad size does and that the resize is recalled
    raw = " ".join(open(os.path.join(ROOT, "include", "bihome.h")).read().split())
    doc = raw[:raw.index("int bh_bank_ingest_u8(")].rsplit("/*", 1)[1]
    for phrase in ("src/data/transforms.py:24-46", ":103-122", "preprocess_offline.py", "UNTOUCHED", "AS RECALLED"):
        assert phrase in doc, phrase


def test_c_entry_point_argument_rules():
    """Checked before any launch (so without a GPU): pointers are never dereferenced here."""
    from bihome_amd import _lib
    f, p = _lib.lib.bh_bank_ingest_u8, ctypes.c_void_p(64)

    def call(src=p, src_off=p, src_hw=p, count=2, bank=p, n_slots=5, first=1, H=6, W=8):
        return f(src, src_off, src_hw, count, bank, n_slots, first, H, W, None)
    for bad in (dict(src=None), dict(src_off=None), dict(src_hw=None), dict(bank=None), dict(count=-1), dict(n_slots=0), dict(n_slots=-2),
                dict(H=0), dict(H=-1), dict(W=0), dict(W=-1), dict(first=-1), dict(first=4), dict(first=5, count=1),
                dict(count=6, first=0), dict(first=2147483647, count=2), dict(count=0, bank=None), dict(count=0, W=0),
                dict(count=0, first=6), dict(count=0, first=-1)):
        assert call(**bad) == BH_E_BADARG, bad
    for ok in (dict(count=0), dict(count=0, first=5), dict(count=0, first=0, n_slots=1, H=1, W=1), dict(count=0, H=5, W=7)):
        assert call(**ok) == BH_OK, ok                                       # no images: nothing launched
    if not torch.cuda.is_available():
        assert call() > 0                                                    # (an accepted call does launch: the launch's own error)
        assert call(first=3) > 0 and call(count=5, first=0) > 0              # the last slots, the whole bank
