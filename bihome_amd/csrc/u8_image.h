// The interleaved uint8 RGB bank image, spelled ONCE for the aligner (csrc/align.hip, ecc.hip, cascade.hip, blend.hip) and the bank
// (csrc/bank.hip): which image sample b reads, how a pixel is loaded, the bilinear sample of a pixel through a homography with its
// validity, the border weight of a blend, the rounding to a byte, the stores of pixels and flags, the patch epilogue and the grid clamp.
// The reason is warp_tap.h's: bh_warp_u8, bh_align_prep_warp_u8 and bh_mosaic_u8 promise ONE sample and ONE `valid` (include/bihome.h),
// and they agree bit for bit on which side of a border a pixel falls because they call one function.
#pragma once
#include <type_traits>
#include "warp_tap.h"

#define U8_MAX_GRID_Y 65535
// gridDim.y for `count` samples: the kernels walk b = blockIdx.y, blockIdx.y + gridDim.y, ...
static inline unsigned u8_grid_y(int count) { return (unsigned)(count < U8_MAX_GRID_Y ? count : U8_MAX_GRID_Y); }

// f(flag...) with every run-time bool as a std::true_type / std::false_type: the way from `bytes` or `vec` to a template argument
template <class F> static void u8_flags(F&& f) { f(); }
template <class F, class... B> static void u8_flags(F&& f, bool v, B... rest) {
    if (v) u8_flags([&](auto... k) { f(std::true_type{}, k...); }, rest...);
    else u8_flags([&](auto... k) { f(std::false_type{}, k...); }, rest...);
}

// sample b's image: idx[b], or b itself without an index list, clamped into [0, n_images) - nothing outside the bank is ever read.
// 64-bit: image 9,321 of a 240 x 320 bank starts past 2^31 bytes.
__device__ __forceinline__ size_t u8_image_index(const int* __restrict__ idx, int b, int n_images) {
    const int i = idx ? idx[b] : b;
    return (size_t)(i < 0 ? 0 : (i >= n_images ? n_images - 1 : i));
}

// The taps are placed by tap_place as in a float plane (offset = 4 * pixel index), and a pixel is read as ONE 4-byte load of any
// alignment, without a branch: bytes 3 p .. 3 p + 3.  The fourth byte belongs to the next pixel - of the next image for the last pixel of
// an image, and outside the buffer for the last pixel of the LAST image, which is therefore read one byte lower and shifted: `lim` is the
// highest byte offset inside the image at which four bytes may be read.  Offsets are 32-bit and relative to the image (3 n < 2^32; the
// image's own base is a 64-bit pointer).  Images of a single pixel take byte loads (BYTES: the caller's compile-time choice, so that the
// common path has no branch at all).
// -> r | g << 8 | b << 16 in bits 0..23; bits 24..31 are NOT pixel data
__device__ __forceinline__ unsigned tap_u8_pixel(unsigned o) { return o == TAP_OUTSIDE ? 0u : o >> 2; }      // a tap outside: pixel 0, weight 0
__device__ __forceinline__ unsigned u8_load_limit(size_t image, int n_images, unsigned n) {
    return image + 1 < (size_t)n_images ? 3u * n - 3u : 3u * n - 4u;      // (n >= 2)
}

struct U8Image { const unsigned char* __restrict__ base; unsigned n, lim; };      // one image of n pixels
__device__ __forceinline__ U8Image u8_image(const unsigned char* __restrict__ images, const int* __restrict__ idx, int b, int n_images, unsigned n) {
    const size_t img = u8_image_index(idx, b, n_images);
    return {images + img * n * 3, n, u8_load_limit(img, n_images, n)};
}
template <bool BYTES>
__device__ __forceinline__ unsigned ld_rgb_u8(const U8Image& im, unsigned pixel) {
    pixel = pixel < im.n ? pixel : im.n - 1u;          // (never past the image, whatever the caller derived the index from)
    if constexpr (BYTES) return (unsigned)im.base[3u * pixel] | ((unsigned)im.base[3u * pixel + 1u] << 8) | ((unsigned)im.base[3u * pixel + 2u] << 16);
    const unsigned off = 3u * pixel, o = off < im.lim ? off : im.lim;
    unsigned v;
    __builtin_memcpy(&v, im.base + o, 4);
    return v >> (8u * (off - o));
}

// The bilinear sample of pixel (x, y) through H in a w x h image, xmax = (float)(w - 1), ymax = (float)(h - 1) (the caller's, computed
// once per kernel and kept in registers it already has).  Taps outside the image contribute 0; under the guard c is unspecified.
// valid: the projected point lies inside [0, w - 1] x [0, h - 1] and was divided.
// The sample comes in two parts, for a kernel that decides from the validity whether it loads at all (csrc/blend.hip): u8_point, the
// projection with the taps placed, and u8_valid are arithmetic only; u8_gather is the four loads and their blend.  u8_sample is the
// composition, the only form every other kernel uses.  (The Tap4 goes by VALUE into both parts: with a reference the compiler schedules
// the kernels that call u8_sample differently; like this their code is instruction for instruction what it was before the split.)
struct U8Sample { float c[3], u, v; bool guard, valid; };
__device__ __forceinline__ Tap4 u8_point(const Hf& H, int x, int y, int w, int h) { return make_tap4(H, x, y, w, h); }
__device__ __forceinline__ bool u8_valid(const Tap4 t, float xmax, float ymax) {
#pragma clang fp contract(off)      // (the comparisons decide validity)
    return !t.guard && t.u >= 0.0f && t.u <= xmax && t.v >= 0.0f && t.v <= ymax;
}
template <bool BYTES>
__device__ __forceinline__ U8Sample u8_gather(const U8Image& im, const Tap4 t, float xmax, float ymax) {
#pragma clang fp contract(off)
    float w00, w01, w10, w11, wsum;
    tap_weights(t, w00, w01, w10, w11, wsum);
    // no branch around the loads: a tap outside the image reads pixel 0 and weighs 0
    const unsigned p00 = ld_rgb_u8<BYTES>(im, tap_u8_pixel(t.o00)), p01 = ld_rgb_u8<BYTES>(im, tap_u8_pixel(t.o01));
    const unsigned p10 = ld_rgb_u8<BYTES>(im, tap_u8_pixel(t.o10)), p11 = ld_rgb_u8<BYTES>(im, tap_u8_pixel(t.o11));
    U8Sample s;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        s.c[c] = tap_blend((float)((p00 >> (8 * c)) & 255u), (float)((p01 >> (8 * c)) & 255u), (float)((p10 >> (8 * c)) & 255u),
                           (float)((p11 >> (8 * c)) & 255u), w00, w01, w10, w11);
    s.u = t.u; s.v = t.v; s.guard = t.guard;
    s.valid = u8_valid(t, xmax, ymax);
    return s;
}
template <bool BYTES>
__device__ __forceinline__ U8Sample u8_sample(const U8Image& im, const Hf& H, int x, int y, int w, int h, float xmax, float ymax) {
    const Tap4 t = u8_point(H, x, y, w, h);
    return u8_gather<BYTES>(im, t, xmax, ymax);
}

// The weight of a sample in a blend (bh_mosaic_u8, bh_pano_u8): min(distance of its projected point to the border of its image + 1,
// feather); meaningful where the sample is valid
__device__ __forceinline__ float u8_border_weight(const U8Sample& s, float xmax, float ymax, float feather) {
#pragma clang fp contract(off)
    return fminf(fminf(fminf(s.u, xmax - s.u), fminf(s.v, ymax - s.v)) + 1.0f, feather);
}
// a feather the blends refuse: NaN, infinite (both fail one of the two comparisons) or below 1
static inline bool u8_feather_bad(float feather) { return !(feather >= 1.0f) || !(feather <= 3.402823466e+38f); }

// round half up into a byte (fmaxf drops a NaN: 0; the conversion truncates)
__device__ __forceinline__ unsigned u8_round(float v) { return (unsigned)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f); }

// PX pixels (3 PX byte values) to dst.  PX = 4: dst on a 4-byte boundary, three dwords (consecutive lanes on consecutive 12 bytes)
struct __attribute__((aligned(4))) Dwords3 { unsigned a, b, c; };
template <int PX>
__device__ __forceinline__ void u8_store_pixels(unsigned char* __restrict__ dst, const unsigned (&o)[PX * 3]) {
    if constexpr (PX == 4) {
        Dwords3 d;
        d.a = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        d.b = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
        d.c = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
        *reinterpret_cast<Dwords3*>(dst) = d;
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) dst[i] = (unsigned char)o[i];
    }
}
// PX one-byte flags to dst; vec: dst is on a 4-byte boundary (PX = 4: one dword)
template <int PX>
__device__ __forceinline__ void u8_store_flags(unsigned char* __restrict__ dst, const unsigned (&f)[PX], int vec) {
    if constexpr (PX == 4) {
        if (vec) { *reinterpret_cast<unsigned*>(dst) = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24); return; }
    }
#pragma unroll
    for (int p = 0; p < PX; ++p) dst[p] = (unsigned char)f[p];
}

// How a blend stores its canvas: vec - Wc % 4 == 0 and out on a 4-byte boundary, a thread makes four pixels (u8_store_pixels<4>), else
// one; flag_vec - the flag plane (NULL ok) is on a 4-byte boundary too (u8_store_flags' vec)
struct U8Stores { bool vec; int flag_vec; };
static inline U8Stores u8_stores(int Wc, const void* out, const void* flags) {
    return {Wc % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0, flags && reinterpret_cast<uintptr_t>(flags) % 4 == 0};
}

// The patch epilogue: channel sums (r, g, b) times inv as gray (C = 1) or per channel (C = 3) in planes pp floats apart, standardised.
// The gray expression is left to the compiler's contraction, as it always was.
template <int C>
__device__ __forceinline__ void u8_store_patch(float* __restrict__ dst, size_t pp, float r, float g, float b, float inv, float mean, float std) {
    if constexpr (C == 1) {
        dst[0] = ((0.299f * r + 0.587f * g + 0.114f * b) * inv - mean) / std;
    } else {
        dst[0] = (r * inv - mean) / std;
        dst[pp] = (g * inv - mean) / std;
        dst[2 * pp] = (b * inv - mean) / std;
    }
}
