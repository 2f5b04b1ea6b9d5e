// Two-band blend of the frames on a canvas (include/bihome.h "Two-band blend"; bihome_amd/align.py holds the numpy float64 statements
// bands_host / mosaic_bands_host the kernels are tested against).  Burt & Adelson's split with two bands, as Brown & Lowe use it: every
// frame comes with its LOW band (bh_blur_u8 of the frame, csrc/blur.hip), the low bands are blended with the wide feather - exposure and
// vignetting fade over the whole overlap - and the HIGH band, value minus low, is taken from ONE frame per pixel, the one with the
// largest border weight, so that frames which disagree by a pixel or two double no edge.
//
// bh_pano_bands_u8: pano.hip's kernel (its tile, pano_tile.h; its wavefront skip; its two store paths) with eight taps per present frame
// instead of four: the frame and its low band are gathered at the SAME Tap4 - one projection, one validity, one weight.
// bh_mosaic_bands_u8: mosaic.hip's kernel for the frames (A, B) of a pair, which may differ in size.
// Both call ONE blend rule (BandAcc, band_add, band_value): for same-size frames the two agree bit for bit.  No LDS, no atomics, no
// scratch, one writer per output element.
#include "u8_image.h"
#include "pano_tile.h"

#define BANDS_MAX_FRAMES 255
#define BANDS_THREADS 256          // the pair's kernel (the sequence's: PANO_THREADS)
#define BANDS_NONE 255u            // winner where nothing is present
#ifndef BANDS_SKIP
#define BANDS_SKIP 1               // 0: every frame takes its taps at every pixel (A/B switch for tools/bands_bench.py)
#endif

// ------------------------------------------------------------------------------------------------
// the blend rule, one pixel
// ------------------------------------------------------------------------------------------------
struct BandAcc { float num[3], den, w_best, v_best[3], l_best[3]; unsigned cnt, winner; };

__device__ __forceinline__ void band_init(BandAcc& a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.num[c] = a.v_best[c] = a.l_best[c] = 0.0f;
    a.den = a.w_best = 0.0f;
    a.cnt = 0u; a.winner = BANDS_NONE;
}
// frame k with value v and low band l (both after the gain) and weight w, in the order k = 0, 1, ...: num += w l with the product rounded
// before it is added, den += w; the frame is the winner if it is the first present or w > w_best, strictly (ties: the lowest k).  A
// frame that is not present is selected out, never multiplied by 0: under the projection guard its sample is unspecified.
__device__ __forceinline__ void band_add(BandAcc& a, bool present, float w, const float (&v)[3], const float (&l)[3], unsigned k) {
#pragma clang fp contract(off)
    const bool take = present && (a.cnt == 0u || w > a.w_best);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float wl = w * l[c];
        a.num[c] = present ? a.num[c] + wl : a.num[c];
        a.v_best[c] = take ? v[c] : a.v_best[c];
        a.l_best[c] = take ? l[c] : a.l_best[c];
    }
    a.den = present ? a.den + w : a.den;
    a.w_best = take ? w : a.w_best;
    a.winner = take ? k : a.winner;
    a.cnt += present ? 1u : 0u;
}
// the value of channel c before rounding: nothing present 0, one frame its own value, else the winner's high band on the blended low band
__device__ __forceinline__ float band_value(const BandAcc& a, int c) {
#pragma clang fp contract(off)
    if (a.cnt == 0u) return 0.0f;
    if (a.cnt == 1u) return a.v_best[c];
    return a.v_best[c] + (a.num[c] / a.den - a.l_best[c]);
}

// a frame and its low band at one Tap4 -> band_add
template <bool BYTES>
__device__ __forceinline__ void band_frame(BandAcc& a, const U8Image& im, const U8Image& lo, const Tap4 t, bool present, float xmax, float ymax,
                                           float feather, float g, float o, unsigned k) {
    const U8Sample s = u8_gather<BYTES>(im, t, xmax, ymax), sl = u8_gather<BYTES>(lo, t, xmax, ymax);
    const float w = u8_border_weight(s, xmax, ymax, feather);
    float v[3], l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[c] = __builtin_fmaf(g, s.c[c], o); l[c] = __builtin_fmaf(g, sl.c[c], o); }
    band_add(a, present, w, v, l, k);
}

// low image `image` of `n_low` (no index list: the low bank is made in the order the blend reads it); 64-bit, nothing clamped
__device__ __forceinline__ U8Image band_low_image(const unsigned char* __restrict__ low, size_t image, size_t n_low, unsigned n) {
    return {low + image * n * 3, n, image + 1 < n_low ? 3u * n - 3u : 3u * n - 4u};
}

// ------------------------------------------------------------------------------------------------
// the sequence
// ------------------------------------------------------------------------------------------------
// grid (pano_grid_x, u8_grid_y(B)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (count_vec / winner_vec: that plane % 4 == 0 too)
template <int PX, bool BYTES>
__global__ void __launch_bounds__(PANO_THREADS) pano_bands_kernel(const unsigned char* __restrict__ images, const unsigned char* __restrict__ low,
                                                                  const int* __restrict__ idx, int n_images, int Hs, int Ws, const double* __restrict__ M64,
                                                                  const double* __restrict__ gain, const unsigned char* __restrict__ use, int B, int n, int Hc,
                                                                  int Wc, float feather, unsigned char* __restrict__ out, unsigned char* __restrict__ count,
                                                                  unsigned char* __restrict__ winner, int count_vec, int winner_vec) {
#pragma clang fp contract(off)
    int x, y;
    if (!pano_unit<PX>(Hc, Wc, x, y)) return;
    const unsigned npix = (unsigned)Hs * (unsigned)Ws;
    const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        BandAcc acc[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) band_init(acc[p]);
        for (int k = 0; k < n; ++k) {
            const size_t f = (size_t)b * n + k;
            if (use && use[f] == 0) continue;                                  // (the same for every lane)
            const Hf M = load_h(M64 + 9 * f);
            Tap4 t[PX];
            bool present[PX], any = false;
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                t[p] = u8_point(M, x + p, y, Ws, Hs);
                present[p] = u8_valid(t[p], xmax, ymax);
                any = any || present[p];
            }
#if BANDS_SKIP
            if (!__any(any)) continue;                                         // absent from the whole wavefront: no load at all
#endif
            const float g = gain ? (float)gain[2 * f] : 1.0f, o = gain ? (float)gain[2 * f + 1] : 0.0f;
            const U8Image im = u8_image(images, idx ? idx + (size_t)b * n : nullptr, k, n_images, npix);
            const U8Image lo = band_low_image(low, f, (size_t)B * n, npix);
#pragma unroll
            for (int p = 0; p < PX; ++p) band_frame<BYTES>(acc[p], im, lo, t[p], present[p], xmax, ymax, feather, g, o, (unsigned)k);
        }
        unsigned q[PX * 3], cnt[PX], win[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) q[p * 3 + c] = u8_round(band_value(acc[p], c));
            cnt[p] = acc[p].cnt; win[p] = acc[p].winner;
        }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        u8_store_pixels<PX>(out + at * 3, q);
        if (count) u8_store_flags<PX>(count + at, cnt, count_vec);
        if (winner) u8_store_flags<PX>(winner + at, win, winner_vec);
    }
}

// ------------------------------------------------------------------------------------------------
// the pair
// ------------------------------------------------------------------------------------------------
// grid (ceil(Hc * (Wc / PX) / BANDS_THREADS), u8_grid_y(B)): mosaic.hip's walk
template <int PX, bool BYTES_A, bool BYTES_B>
__global__ void __launch_bounds__(BANDS_THREADS) mosaic_bands_kernel(const unsigned char* __restrict__ images_a, const unsigned char* __restrict__ low_a,
                                                                     const int* __restrict__ idx_a, int n_a, int Ha, int Wa,
                                                                     const unsigned char* __restrict__ images_b, const unsigned char* __restrict__ low_b,
                                                                     const int* __restrict__ idx_b, int n_b, int Hb, int Wb, const double* __restrict__ Ma64,
                                                                     const double* __restrict__ Mb64, const double* __restrict__ gain, int B, int Hc, int Wc,
                                                                     float feather, unsigned char* __restrict__ out, unsigned char* __restrict__ cover,
                                                                     unsigned char* __restrict__ winner, int cover_vec, int winner_vec) {
    const unsigned upr = (unsigned)Wc / PX;                                    // units per canvas row
    const unsigned u = blockIdx.x * BANDS_THREADS + threadIdx.x;
    if (u >= upr * (unsigned)Hc) return;
    const int y = (int)(u / upr), x = (int)(u - (unsigned)y * upr) * PX;
    const unsigned na = (unsigned)Ha * (unsigned)Wa, nb = (unsigned)Hb * (unsigned)Wb;
    const float xmax_a = (float)(Wa - 1), ymax_a = (float)(Ha - 1), xmax_b = (float)(Wb - 1), ymax_b = (float)(Hb - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Hf Ma = load_h(Ma64 + 9 * (size_t)b), Mb = load_h(Mb64 + 9 * (size_t)b);
        const float g = gain ? (float)gain[2 * (size_t)b] : 1.0f, o = gain ? (float)gain[2 * (size_t)b + 1] : 0.0f;
        const U8Image im_a = u8_image(images_a, idx_a, b, n_a, na), im_b = u8_image(images_b, idx_b, b, n_b, nb);
        const U8Image lo_a = band_low_image(low_a, (size_t)b, (size_t)B, na), lo_b = band_low_image(low_b, (size_t)b, (size_t)B, nb);
        unsigned q[PX * 3], code[PX], win[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            BandAcc acc;
            band_init(acc);
            const Tap4 ta = u8_point(Ma, x + p, y, Wa, Ha), tb = u8_point(Mb, x + p, y, Wb, Hb);
            const bool pa = u8_valid(ta, xmax_a, ymax_a), pb = u8_valid(tb, xmax_b, ymax_b);
            band_frame<BYTES_A>(acc, im_a, lo_a, ta, pa, xmax_a, ymax_a, feather, g, o, 0u);
            band_frame<BYTES_B>(acc, im_b, lo_b, tb, pb, xmax_b, ymax_b, feather, 1.0f, 0.0f, 1u);
#pragma unroll
            for (int c = 0; c < 3; ++c) q[p * 3 + c] = u8_round(band_value(acc, c));
            code[p] = (pa ? 1u : 0u) | (pb ? 2u : 0u);
            win[p] = acc.winner;
        }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        u8_store_pixels<PX>(out + at * 3, q);
        if (cover) u8_store_flags<PX>(cover + at, code, cover_vec);
        if (winner) u8_store_flags<PX>(winner + at, win, winner_vec);
    }
}

// what the entry points refuse as BH_E_BADARG apart from their NULL pointers and the feather: bh_pano_u8's and bh_mosaic_u8's rules
static bool bands_counts_bad(int count, int frames) { return count < 0 || frames < 1 || frames > BANDS_MAX_FRAMES; }
static bool bands_extent_bad(int n_images, int Hs, int Ws) { return n_images < 1 || Hs < 1 || Ws < 1; }
static int bands_plane_vec(const void* plane) { return plane && reinterpret_cast<uintptr_t>(plane) % 4 == 0; }

extern "C" {

int bh_pano_bands_u8(const uint8_t* images, const uint8_t* low, const int* idx, int n_images, int Hs, int Ws, const double* M, const double* gain,
                     const uint8_t* use, int B, int n, int Hc, int Wc, float feather, uint8_t* out, uint8_t* count, uint8_t* winner, void* stream) {
    if (!images || !low || !M || !out || bands_counts_bad(B, n) || bands_extent_bad(n_images, Hs, Ws) || Hc < 1 || Wc < 1) return BH_E_BADARG;
    if (u8_feather_bad(feather)) return BH_E_BADARG;
    // (bh_pano_u8's limits: tap_place's offsets, 32-bit byte offsets inside an image, the unit index of a thread)
    if ((long long)Hs * Ws > (1ll << 29) || (long long)Hc * Wc > 0x7fffffffll) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const U8Stores stores = u8_stores(Wc, out, count);
    const dim3 grid(pano_grid_x(Hc, Wc, stores.vec ? 4 : 1), u8_grid_y(B));
    hipStream_t st = bh_stream(stream);
    const bool bytes = (long long)Hs * Ws < 2;                                 // a single-pixel frame: no room for 4-byte loads
    u8_flags([&](auto four, auto by) {
        hipLaunchKernelGGL((pano_bands_kernel<four ? 4 : 1, by>), grid, dim3(PANO_THREADS), 0, st, images, low, idx, n_images, Hs, Ws, M, gain, use, B, n, Hc, Wc,
                           feather, out, count, winner, stores.flag_vec, bands_plane_vec(winner));
    }, stores.vec, bytes);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_mosaic_bands_u8(const uint8_t* images_a, const uint8_t* low_a, const int* idx_a, int n_a, int Ha, int Wa,
                       const uint8_t* images_b, const uint8_t* low_b, const int* idx_b, int n_b, int Hb, int Wb,
                       const double* Ma, const double* Mb, const double* gain,
                       int B, int Hc, int Wc, float feather,
                       uint8_t* out, uint8_t* cover, uint8_t* winner, void* stream) {
    if (!images_a || !low_a || !images_b || !low_b || !Ma || !Mb || !out) return BH_E_BADARG;
    if (bands_counts_bad(B, 2) || bands_extent_bad(n_a, Ha, Wa) || bands_extent_bad(n_b, Hb, Wb) || Hc < 1 || Wc < 1) return BH_E_BADARG;
    if (u8_feather_bad(feather)) return BH_E_BADARG;
    // (bh_mosaic_u8's limits)
    if ((long long)Ha * Wa > (1ll << 29) || (long long)Hb * Wb > (1ll << 29) || (long long)Hc * Wc > 0x7fffffffll) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const U8Stores stores = u8_stores(Wc, out, cover);
    const unsigned units = (unsigned)Hc * ((unsigned)Wc / (stores.vec ? 4 : 1));
    const dim3 grid((units + BANDS_THREADS - 1) / BANDS_THREADS, u8_grid_y(B));
    hipStream_t st = bh_stream(stream);
    const bool ba = (long long)Ha * Wa < 2, bb = (long long)Hb * Wb < 2;       // a single-pixel image: no room for 4-byte loads
    u8_flags([&](auto four, auto by_a, auto by_b) {
        hipLaunchKernelGGL((mosaic_bands_kernel<four ? 4 : 1, by_a, by_b>), grid, dim3(BANDS_THREADS), 0, st, images_a, low_a, idx_a, n_a, Ha, Wa, images_b, low_b,
                           idx_b, n_b, Hb, Wb, Ma, Mb, gain, B, Hc, Wc, feather, out, cover, winner, stores.flag_vec, bands_plane_vec(winner));
    }, stores.vec, ba, bb);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
