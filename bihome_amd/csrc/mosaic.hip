// Mosaic: both images of an aligned pair on one canvas, feathered, in one pass (include/bihome.h "Mosaic"; bihome_amd/align.py holds the
// numpy float64 statement mosaic_host the kernel is tested against).
//
// bh_mosaic_u8: canvas pixel (x, y) projects through Ma into image A and through Mb into image B - u8_image.h's u8_sample, so the
// values and the `valid` are the ones bh_warp_u8 makes - takes the four taps of each (eight 4-byte loads of any alignment), applies the
// gain / bias to A's value, weighs each image by the distance of its projected point to the border of the image plus 1, capped at
// `feather`, blends (or, in the two "over" modes, selects), rounds half up and stores.  An image that is not present at a pixel is
// selected out, never multiplied by 0: under the projection guard its sample is unspecified.  No full-size intermediate, no atomics, no
// scratch, no LDS, one writer per output element.  The weight (u8_border_weight), the feather rule and the choice between the two store
// paths are u8_image.h's, shared with pano.hip; the fitted canvas itself is pano.hip's bh_pano_frame with A as its single frame
// (align.py mosaic_frame_device).
//
// Wc % 4 == 0 and out on a 4-byte boundary: a thread makes four pixels and stores three dwords (consecutive lanes on consecutive
// 12 bytes, u8_store_pixels) and, with cover on a 4-byte boundary, one dword of cover codes (u8_store_flags); anything else: one pixel,
// byte stores.  The offset of an image in its bank is 64-bit, offsets inside an image 32-bit, the image index is clamped and so is every
// pixel index (u8_image.h).
#include "u8_image.h"

#define MOSAIC_THREADS 256

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

// grid (ceil(Hc * (Wc / PX) / MOSAIC_THREADS), u8_grid_y(B)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (cover_vec: cover % 4 == 0 too)
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
        const U8Image im_a = u8_image(images_a, idx_a, b, n_a, na), im_b = u8_image(images_b, idx_b, b, n_b, nb);
        unsigned q[PX * 3], code[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const U8Sample sa = u8_sample<BYTES_A>(im_a, Ma, x + p, y, Wa, Ha, xmax_a, ymax_a);
            const U8Sample sb = u8_sample<BYTES_B>(im_b, Mb, x + p, y, Wb, Hb, xmax_b, ymax_b);
            const float wa = u8_border_weight(sa, xmax_a, ymax_a, feather), wb = u8_border_weight(sb, xmax_b, ymax_b, feather);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                q[p * 3 + c] = u8_round(mosaic_value(__builtin_fmaf(g, sa.c[c], o), sb.c[c], wa, wb, sa.valid, sb.valid, mode));
            code[p] = (sa.valid ? 1u : 0u) | (sb.valid ? 2u : 0u);
        }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        u8_store_pixels<PX>(out + at * 3, q);
        if (cover) u8_store_flags<PX>(cover + at, code, cover_vec);
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
    if (u8_feather_bad(feather)) return BH_E_BADARG;
    if (mode != BH_MOSAIC_FEATHER && mode != BH_MOSAIC_B_OVER_A && mode != BH_MOSAIC_A_OVER_B) return BH_E_BADARG;
    // (tap_place's offsets are ints of 4 bytes per pixel, byte offsets inside an image 32-bit; the unit index of a thread is an unsigned)
    if ((long long)Ha * Wa > (1ll << 29) || (long long)Hb * Wb > (1ll << 29) || (long long)Hc * Wc > 0x7fffffffll) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const U8Stores stores = u8_stores(Wc, out, cover);
    const unsigned units = (unsigned)Hc * ((unsigned)Wc / (stores.vec ? 4 : 1));
    const dim3 grid((units + MOSAIC_THREADS - 1) / MOSAIC_THREADS, u8_grid_y(B));
    hipStream_t st = bh_stream(stream);
    const bool ba = (long long)Ha * Wa < 2, bb = (long long)Hb * Wb < 2;       // a single-pixel image: no room for 4-byte loads
    u8_flags([&](auto four, auto by_a, auto by_b) {
        hipLaunchKernelGGL((mosaic_kernel<four ? 4 : 1, by_a, by_b>), grid, dim3(MOSAIC_THREADS), 0, st, images_a, idx_a, n_a, Ha, Wa, images_b, idx_b, n_b, Hb, Wb,
                           Ma, Mb, gain, B, Hc, Wc, feather, mode, out, cover, stores.flag_vec);
    }, stores.vec, ba, bb);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
