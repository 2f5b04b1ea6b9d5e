// Mosaic: both images of an aligned pair on one canvas, feathered, in one pass (include/bihome.h "Mosaic"; bihome_amd/align.py holds the
// numpy float64 statement mosaic_host the kernel is tested against).
//
// bh_mosaic_u8: canvas pixel (x, y) projects through Ma into image A and through Mb into image B - warp_tap.h's make_tap4, so the pixels
// sampled are the pixels bh_warp_u8 samples - takes the four taps of each (eight 4-byte loads of any alignment, ld_rgb_u8), applies the
// gain / bias to A's value, weighs each image by the distance of its projected point to the border of the image plus 1, capped at
// `feather`, blends (or, in the two "over" modes, selects), rounds half up and stores.  An image that is not present at a pixel is
// selected out, never multiplied by 0: under the projection guard its sample is unspecified.  No full-size intermediate, no atomics, no
// scratch, no LDS, one writer per output element.
//
// Wc % 4 == 0 and out on a 4-byte boundary: a thread makes four pixels and stores three dwords (consecutive lanes on consecutive
// 12 bytes, align.hip's layout) and, with cover on a 4-byte boundary, one dword of cover codes; anything else: one pixel, byte stores.
// The offset of an image in its bank is 64-bit, offsets inside an image 32-bit, the image index is clamped and so is every pixel index.
#include "warp_tap.h"

#define MOSAIC_THREADS 256
#define MOSAIC_MAX_GRID_Y 65535

struct __attribute__((aligned(4))) MosaicDwords3 { unsigned a, b, c; };

// sample b's image: idx[b], or b itself without an index list, clamped into [0, n_images)
__device__ __forceinline__ size_t mosaic_image(const int* __restrict__ idx, int b, int n_images) {
    const int i = idx ? idx[b] : b;
    return (size_t)(i < 0 ? 0 : (i >= n_images ? n_images - 1 : i));
}

struct MosaicSample {
    float c[3];        // the bilinear value per channel, taps outside the image 0 (unspecified under the guard)
    float w;           // min(distance to the border + 1, feather); meaningful where present
    bool present;      // bh_warp_u8's `valid`
};

template <bool BYTES>
__device__ __forceinline__ MosaicSample mosaic_sample(const unsigned char* __restrict__ image, unsigned n, unsigned lim, const Hf& M, int x, int y,
                                                      int W, int H, float xmax, float ymax, float feather) {
#pragma clang fp contract(off)      // (the comparisons below decide presence)
    const Tap4 t = make_tap4(M, x, y, W, H);
    float w00, w01, w10, w11, wsum;
    tap_weights(t, w00, w01, w10, w11, wsum);
    // no branch around the loads: a tap outside the image reads pixel 0 and weighs 0
    const unsigned p00 = ld_rgb_u8<BYTES>(image, tap_u8_pixel(t.o00), n, lim), p01 = ld_rgb_u8<BYTES>(image, tap_u8_pixel(t.o01), n, lim);
    const unsigned p10 = ld_rgb_u8<BYTES>(image, tap_u8_pixel(t.o10), n, lim), p11 = ld_rgb_u8<BYTES>(image, tap_u8_pixel(t.o11), n, lim);
    MosaicSample s;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        s.c[c] = tap_blend((float)((p00 >> (8 * c)) & 255u), (float)((p01 >> (8 * c)) & 255u), (float)((p10 >> (8 * c)) & 255u),
                           (float)((p11 >> (8 * c)) & 255u), w00, w01, w10, w11);
    s.present = !t.guard && t.u >= 0.0f && t.u <= xmax && t.v >= 0.0f && t.v <= ymax;
    s.w = fminf(fminf(fminf(t.u, xmax - t.u), fminf(t.v, ymax - t.v)) + 1.0f, feather);
    return s;
}

// the value of one channel before rounding: a is A's value after the gain
__device__ __forceinline__ float mosaic_value(float a, float b, float wa, float wb, bool pa, bool pb, int mode) {
#pragma clang fp contract(off)
    if (mode == BH_MOSAIC_FEATHER) {
        const float num = (pa ? wa * a : 0.0f) + (pb ? wb * b : 0.0f), den = (pa ? wa : 0.0f) + (pb ? wb : 0.0f);
        return den > 0.0f ? num / den : 0.0f;
    }
    if (mode == BH_MOSAIC_B_OVER_A) return pb ? b : (pa ? a : 0.0f);
    return pa ? a : (pb ? b : 0.0f);
}

// grid (ceil(Hc * (Wc / PX) / MOSAIC_THREADS), min(B, MOSAIC_MAX_GRID_Y)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (cover_vec: cover % 4 == 0 too)
template <int PX, bool BYTES_A, bool BYTES_B>
__global__ void __launch_bounds__(MOSAIC_THREADS) mosaic_kernel(const unsigned char* __restrict__ images_a, const int* __restrict__ idx_a, int n_a, int Ha, int Wa,
                                                                const unsigned char* __restrict__ images_b, const int* __restrict__ idx_b, int n_b, int Hb, int Wb,
                                                                const double* __restrict__ Ma64, const double* __restrict__ Mb64, const double* __restrict__ gain,
                                                                int B, int Hc, int Wc, float feather, int mode,
                                                                unsigned char* __restrict__ out, unsigned char* __restrict__ cover, int cover_vec) {
    const unsigned upr = (unsigned)Wc / PX;                                    // units per canvas row
    const unsigned u = blockIdx.x * MOSAIC_THREADS + threadIdx.x;
    if (u >= upr * (unsigned)Hc) return;
    const int y = (int)(u / upr), x = (int)(u - (unsigned)y * upr) * PX;
    const unsigned na = (unsigned)Ha * (unsigned)Wa, nb = (unsigned)Hb * (unsigned)Wb;
    const float xmax_a = (float)(Wa - 1), ymax_a = (float)(Ha - 1), xmax_b = (float)(Wb - 1), ymax_b = (float)(Hb - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Hf Ma = load_h(Ma64 + 9 * (size_t)b), Mb = load_h(Mb64 + 9 * (size_t)b);
        const float g = gain ? (float)gain[2 * (size_t)b] : 1.0f, o = gain ? (float)gain[2 * (size_t)b + 1] : 0.0f;
        const size_t ia = mosaic_image(idx_a, b, n_a), ib = mosaic_image(idx_b, b, n_b);
        const unsigned char* image_a = images_a + ia * na * 3;
        const unsigned char* image_b = images_b + ib * nb * 3;
        const unsigned lim_a = u8_load_limit(ia, n_a, na), lim_b = u8_load_limit(ib, n_b, nb);
        unsigned q[PX * 3], code[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const MosaicSample sa = mosaic_sample<BYTES_A>(image_a, na, lim_a, Ma, x + p, y, Wa, Ha, xmax_a, ymax_a, feather);
            const MosaicSample sb = mosaic_sample<BYTES_B>(image_b, nb, lim_b, Mb, x + p, y, Wb, Hb, xmax_b, ymax_b, feather);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = mosaic_value(__builtin_fmaf(g, sa.c[c], o), sb.c[c], sa.w, sb.w, sa.present, sb.present, mode);
                q[p * 3 + c] = (unsigned)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f);      // (fmaxf drops a NaN: 0) round half up: the conversion truncates
            }
            code[p] = (sa.present ? 1u : 0u) | (sb.present ? 2u : 0u);
        }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        unsigned char* dst = out + at * 3;
        if constexpr (PX == 4) {
            MosaicDwords3 d;
            d.a = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            d.b = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
            d.c = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
            *reinterpret_cast<MosaicDwords3*>(dst) = d;
            if (cover) {
                if (cover_vec) *reinterpret_cast<unsigned*>(cover + at) = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
                else {
#pragma unroll
                    for (int p = 0; p < 4; ++p) cover[at + p] = (unsigned char)code[p];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) dst[i] = (unsigned char)q[i];
            if (cover) cover[at] = (unsigned char)code[0];
        }
    }
}

// what the entry point refuses as BH_E_BADARG apart from its NULL pointers, feather and mode: a negative batch, a bank / image / canvas without extent
static bool mosaic_extents_bad(int count, int n_a, int Ha, int Wa, int n_b, int Hb, int Wb, int Hc, int Wc) {
    return count < 0 || n_a < 1 || Ha < 1 || Wa < 1 || n_b < 1 || Hb < 1 || Wb < 1 || Hc < 1 || Wc < 1;
}

extern "C" {

int bh_mosaic_u8(const uint8_t* images_a, const int* idx_a, int n_a, int Ha, int Wa,
                 const uint8_t* images_b, const int* idx_b, int n_b, int Hb, int Wb,
                 const double* Ma, const double* Mb, const double* gain,
                 int B, int Hc, int Wc, float feather, int mode,
                 uint8_t* out, uint8_t* cover, void* stream) {
    if (!images_a || !images_b || !Ma || !Mb || !out || mosaic_extents_bad(B, n_a, Ha, Wa, n_b, Hb, Wb, Hc, Wc)) return BH_E_BADARG;
    if (!(feather >= 1.0f) || !(feather <= 3.402823466e+38f)) return BH_E_BADARG;                  // (NaN and infinity fail one of the two)
    if (mode != BH_MOSAIC_FEATHER && mode != BH_MOSAIC_B_OVER_A && mode != BH_MOSAIC_A_OVER_B) return BH_E_BADARG;
    // (tap_place's offsets are ints of 4 bytes per pixel, byte offsets inside an image 32-bit; the unit index of a thread is an unsigned)
    if ((long long)Ha * Wa > (1ll << 29) || (long long)Hb * Wb > (1ll << 29) || (long long)Hc * Wc > 0x7fffffffll) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const bool vec = Wc % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const int cover_vec = cover && reinterpret_cast<uintptr_t>(cover) % 4 == 0;
    const unsigned units = (unsigned)Hc * ((unsigned)Wc / (vec ? 4 : 1));
    const dim3 grid((units + MOSAIC_THREADS - 1) / MOSAIC_THREADS, (unsigned)(B < MOSAIC_MAX_GRID_Y ? B : MOSAIC_MAX_GRID_Y));
    hipStream_t st = bh_stream(stream);
    const bool ba = (long long)Ha * Wa < 2, bb = (long long)Hb * Wb < 2;       // a single-pixel image: no room for 4-byte loads
#define MOSAIC_LAUNCH(PX_, BA_, BB_) hipLaunchKernelGGL((mosaic_kernel<PX_, BA_, BB_>), grid, dim3(MOSAIC_THREADS), 0, st, images_a, idx_a, n_a, Ha, Wa, \
                                                        images_b, idx_b, n_b, Hb, Wb, Ma, Mb, gain, B, Hc, Wc, feather, mode, out, cover, cover_vec)
#define MOSAIC_BYTES(PX_) do { if (ba) { if (bb) MOSAIC_LAUNCH(PX_, true, true); else MOSAIC_LAUNCH(PX_, true, false); } \
                               else { if (bb) MOSAIC_LAUNCH(PX_, false, true); else MOSAIC_LAUNCH(PX_, false, false); } } while (0)
    if (vec) MOSAIC_BYTES(4); else MOSAIC_BYTES(1);
#undef MOSAIC_BYTES
#undef MOSAIC_LAUNCH
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
