// The blends of the aligner's canvas stage: frames on one canvas, in one pass (include/bihome.h "Mosaic", "Panorama", "Two-band blend";
// bihome_amd/align.py holds the numpy float64 statements mosaic_host / pano_host / bands_host / mosaic_bands_host the kernels are tested
// against).  Two canvas walks and two blend rules:
//
//                                   the sequence walk                        the pair walk
//   feather / first / last          bh_pano_u8 (pano_kernel)                 bh_mosaic_u8 (mosaic_kernel, mosaic_value)
//   two-band (BandRule)             bh_pano_bands_u8 (blend_seq_kernel)      bh_mosaic_bands_u8 (blend_pair_kernel)
//
// A walk is which canvas pixels a thread makes and which frames it visits.  Canvas pixel (x, y) projects through a frame's M into the frame
// - u8_image.h's u8_point / u8_valid / u8_gather, so the values and the `valid` are the ones bh_warp_u8 makes - takes the four taps (4-byte
// loads of any alignment), applies the gain / bias, blends, rounds half up and stores.
//   The sequence: n frames of ONE bank and one size, a run-time loop.  Per frame a thread first projects its pixels (arithmetic only), and
//     when no lane of the wavefront has the frame present the wavefront goes on to the next frame without a single load (PANO_SKIP) - in a
//     pan most canvas pixels see 0 to 3 of the n frames.  That cannot change a result.  The pixels of a wavefront are a compact tile, not a
//     run of one row, because a tile is absent from more frames (PANO_TILE; pano_unit).  The flag plane is the number of frames present.
//   The pair: the frames (A, B) of two banks, which may differ in size, the gain on A only; consecutive threads on consecutive units of
//     one row (row_unit), pixels outer and the two frames inner, no skip.  The flag plane is the cover code (A present) | (B present) << 1.
// A rule is how the frames present at a pixel become its value, in the order k = 0, 1, ...: every product is rounded before it is added,
// and a frame that is not present is selected out, never multiplied by 0 (under the projection guard its sample is unspecified).  So
// n = 2 of a sequence equals the pair bit for bit, and the two-band blend with one frame present equals mode "first".
//   feather / first / last: a frame's weight is the distance of its projected point to the border of the frame plus 1, capped at `feather`
//     (u8_image.h's u8_border_weight); num += w v, den += w, or the value of the first / last frame present (the run-time `mode`).
//   two-band: Burt & Adelson's split with two bands, as Brown & Lowe use it.  Every frame comes with its LOW band (bh_blur_u8 of the frame,
//     csrc/blur.hip); the low bands are blended with the wide feather - exposure and vignetting fade over the whole overlap - and the HIGH
//     band, value minus low, is taken from ONE frame per pixel, the one with the largest border weight, so that frames which disagree by a
//     pixel or two double no edge.  The frame and its low band are gathered at the SAME Tap4: one projection, one validity, one weight.
// The two-band rule is ONE struct (BandRule: the accumulator of a pixel with init, add(present, w, v, l, k), value(c)) and its two kernels
// are the two walks as templates over the rule.  The feather rule is written into its two kernels, once as the accumulator and once as the
// closed form of n = 2: as a second rule struct behind the same templates it made the same bits but ran slower (the note above pano_kernel).
// The unit of a thread, the refusals, the size limits, the choice of the store path, the grid and the launch check are written once per
// walk (row_unit / pano_unit, blend_refuse, blend_seq, blend_pair) and serve both rules.
// Wc % 4 == 0 and out on a 4-byte boundary: a thread makes four pixels and stores three dwords (consecutive lanes on consecutive
// 12 bytes, u8_store_pixels) and, with a flag plane on a 4-byte boundary, one dword of flags (u8_store_flags); anything else: one pixel,
// byte stores.  The offset of an image in its bank is 64-bit, offsets inside an image 32-bit, the image index is clamped and so is every
// pixel index (u8_image.h).  No full-size intermediate, no LDS, no atomics, no scratch, one writer per output element.  The fitted canvas
// itself is pano.hip's bh_pano_frame.
#include "u8_image.h"

#define BLEND_THREADS 256
#define BLEND_MAX_FRAMES 255
#define BLEND_NONE 255u            // winner where nothing is present
// A/B switches for tools/pano_bench.py and tools/bands_bench.py (make ab ABFLAGS=-DPANO_SKIP=0 / -DPANO_TILE=0); DESIGN.md section 8
// "Panorama" has the figures
#ifndef PANO_SKIP
#define PANO_SKIP 1        // 0: every frame takes its taps at every pixel
#endif
#ifndef PANO_TILE
#define PANO_TILE 1        // 1: a wavefront makes 8 units x 8 rows of the canvas (a unit: 4 pixels, or 1), a workgroup 32 units x 8 rows - the
#endif                     // compact tile is absent from more frames; 0: the pair's 64 consecutive units of one row (longer store runs)

// ------------------------------------------------------------------------------------------------
// the two-band rule, one pixel
// ------------------------------------------------------------------------------------------------
// frame k with value v and low band l (both after the gain) and weight w: num += w l with the product rounded before it is added,
// den += w; the frame is the winner if it is the first present or w > w_best, strictly (ties: the lowest k)
struct BandRule {
    float num[3], den, w_best, v_best[3], l_best[3];
    unsigned cnt, winner;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int c = 0; c < 3; ++c) num[c] = v_best[c] = l_best[c] = 0.0f;
        den = w_best = 0.0f;
        cnt = 0u; winner = BLEND_NONE;
    }
    __device__ __forceinline__ void add(bool present, float w, const float (&v)[3], const float (&l)[3], unsigned k) {
#pragma clang fp contract(off)
        const bool take = present && (cnt == 0u || w > w_best);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float wl = w * l[c];
            num[c] = present ? num[c] + wl : num[c];
            v_best[c] = take ? v[c] : v_best[c];
            l_best[c] = take ? l[c] : l_best[c];
        }
        den = present ? den + w : den;
        w_best = take ? w : w_best;
        winner = take ? k : winner;
        cnt += present ? 1u : 0u;
    }
    // the value of channel c before rounding: nothing present 0, one frame its own value, else the winner's high band on the blended low band
    __device__ __forceinline__ float value(int c) const {
#pragma clang fp contract(off)
        if (cnt == 0u) return 0.0f;
        if (cnt == 1u) return v_best[c];
        return v_best[c] + (num[c] / den - l_best[c]);
    }
};

// frame k at one Tap4 -> the rule: the four taps of the frame and of its low band `lo`, the border weight, the gain
template <bool BYTES, class Rule>
__device__ __forceinline__ void blend_frame(Rule& a, const U8Image& im, const U8Image& lo, const Tap4 t, bool present, float xmax, float ymax,
                                            float feather, float g, float o, unsigned k) {
    const U8Sample s = u8_gather<BYTES>(im, t, xmax, ymax), sl = u8_gather<BYTES>(lo, t, xmax, ymax);
    const float w = u8_border_weight(s, xmax, ymax, feather);
    float v[3], l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[c] = __builtin_fmaf(g, s.c[c], o); l[c] = __builtin_fmaf(g, sl.c[c], o); }
    a.add(present, w, v, l, k);
}

// low image `image` of `n_low` (no index list: the low bank is made in the order the blend reads it); 64-bit, nothing clamped
__device__ __forceinline__ U8Image blend_low_image(const unsigned char* __restrict__ low, size_t image, size_t n_low, unsigned n) {
    return {low + image * n * 3, n, image + 1 < n_low ? 3u * n - 3u : 3u * n - 4u};
}

// ------------------------------------------------------------------------------------------------
// which unit of PX pixels a thread makes -> (x, y) of its first pixel; false: outside the canvas
// ------------------------------------------------------------------------------------------------
// consecutive threads on consecutive units of one row: grid.x = row_grid_x
template <int PX>
__device__ __forceinline__ bool row_unit(int Hc, int Wc, int& x, int& y) {
    const unsigned upr = (unsigned)Wc / PX;                                    // units per canvas row
    const unsigned u = blockIdx.x * BLEND_THREADS + threadIdx.x;
    if (u >= upr * (unsigned)Hc) return false;
    y = (int)(u / upr); x = (int)(u - (unsigned)y * upr) * PX;
    return true;
}
static unsigned row_grid_x(int Hc, int Wc, int px) { return ((unsigned)Wc / px * (unsigned)Hc + BLEND_THREADS - 1) / BLEND_THREADS; }

// the sequence's compact tile (PANO_TILE): grid.x = pano_grid_x
template <int PX>
__device__ __forceinline__ bool pano_unit(int Hc, int Wc, int& x, int& y) {
#if PANO_TILE
    const unsigned upr = (unsigned)Wc / PX;
    const unsigned tiles_x = (upr + 31u) / 32u, by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const unsigned ux = bx * 32u + (threadIdx.x >> 6) * 8u + (threadIdx.x & 7u), uy = by * 8u + ((threadIdx.x >> 3) & 7u);
    if (ux >= upr || uy >= (unsigned)Hc) return false;
    x = (int)ux * PX; y = (int)uy;
    return true;
#else
    return row_unit<PX>(Hc, Wc, x, y);
#endif
}
static unsigned pano_grid_x(int Hc, int Wc, int px) {
#if PANO_TILE
    return (((unsigned)Wc / px + 31u) / 32u) * (((unsigned)Hc + 7u) / 8u);
#else
    return row_grid_x(Hc, Wc, px);
#endif
}

// ------------------------------------------------------------------------------------------------
// the sequence walk
// ------------------------------------------------------------------------------------------------
// grid (pano_grid_x, u8_grid_y(B)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (count_vec / winner_vec: that plane % 4 == 0 too).  low, winner:
// the low bank the rule reads and the plane of its winners
template <class Rule, int PX, bool BYTES>
__global__ void __launch_bounds__(BLEND_THREADS) blend_seq_kernel(const unsigned char* __restrict__ images, const unsigned char* __restrict__ low,
                                                                  const int* __restrict__ idx, int n_images, int Hs, int Ws, const double* __restrict__ M64,
                                                                  const double* __restrict__ gain, const unsigned char* __restrict__ use, int B, int n, int Hc,
                                                                  int Wc, float feather, unsigned char* __restrict__ out,
                                                                  unsigned char* __restrict__ count, unsigned char* __restrict__ winner, int count_vec,
                                                                  int winner_vec) {
#pragma clang fp contract(off)
    int x, y;
    if (!pano_unit<PX>(Hc, Wc, x, y)) return;
    const unsigned npix = (unsigned)Hs * (unsigned)Ws;
    const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        Rule acc[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) acc[p].init();
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
#if PANO_SKIP
            if (!__any(any)) continue;                                         // absent from the whole wavefront: no load at all
#endif
            const float g = gain ? (float)gain[2 * f] : 1.0f, o = gain ? (float)gain[2 * f + 1] : 0.0f;
            const U8Image im = u8_image(images, idx ? idx + (size_t)b * n : nullptr, k, n_images, npix);
            const U8Image lo = blend_low_image(low, f, (size_t)B * n, npix);
#pragma unroll
            for (int p = 0; p < PX; ++p) blend_frame<BYTES>(acc[p], im, lo, t[p], present[p], xmax, ymax, feather, g, o, (unsigned)k);
        }
        unsigned q[PX * 3], cnt[PX], win[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) q[p * 3 + c] = u8_round(acc[p].value(c));
            cnt[p] = acc[p].cnt; win[p] = acc[p].winner;
        }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        u8_store_pixels<PX>(out + at * 3, q);
        if (count) u8_store_flags<PX>(count + at, cnt, count_vec);
        if (winner) u8_store_flags<PX>(winner + at, win, winner_vec);
    }
}

// ------------------------------------------------------------------------------------------------
// the pair walk
// ------------------------------------------------------------------------------------------------
// grid (row_grid_x, u8_grid_y(B)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (cover_vec / winner_vec: that plane % 4 == 0 too).  low_a, low_b,
// winner: as in the sequence walk
template <class Rule, int PX, bool BYTES_A, bool BYTES_B>
__global__ void __launch_bounds__(BLEND_THREADS) blend_pair_kernel(const unsigned char* __restrict__ images_a, const unsigned char* __restrict__ low_a,
                                                                   const int* __restrict__ idx_a, int n_a, int Ha, int Wa,
                                                                   const unsigned char* __restrict__ images_b, const unsigned char* __restrict__ low_b,
                                                                   const int* __restrict__ idx_b, int n_b, int Hb, int Wb, const double* __restrict__ Ma64,
                                                                   const double* __restrict__ Mb64, const double* __restrict__ gain, int B, int Hc, int Wc,
                                                                   float feather, unsigned char* __restrict__ out, unsigned char* __restrict__ cover,
                                                                   unsigned char* __restrict__ winner, int cover_vec, int winner_vec) {
    int x, y;
    if (!row_unit<PX>(Hc, Wc, x, y)) return;
    const unsigned na = (unsigned)Ha * (unsigned)Wa, nb = (unsigned)Hb * (unsigned)Wb;
    const float xmax_a = (float)(Wa - 1), ymax_a = (float)(Ha - 1), xmax_b = (float)(Wb - 1), ymax_b = (float)(Hb - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Hf Ma = load_h(Ma64 + 9 * (size_t)b), Mb = load_h(Mb64 + 9 * (size_t)b);
        const float g = gain ? (float)gain[2 * (size_t)b] : 1.0f, o = gain ? (float)gain[2 * (size_t)b + 1] : 0.0f;
        const U8Image im_a = u8_image(images_a, idx_a, b, n_a, na), im_b = u8_image(images_b, idx_b, b, n_b, nb);
        const U8Image lo_a = blend_low_image(low_a, (size_t)b, (size_t)B, na), lo_b = blend_low_image(low_b, (size_t)b, (size_t)B, nb);
        unsigned q[PX * 3], code[PX], win[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            Rule acc;
            acc.init();
            const Tap4 ta = u8_point(Ma, x + p, y, Wa, Ha), tb = u8_point(Mb, x + p, y, Wb, Hb);
            const bool pa = u8_valid(ta, xmax_a, ymax_a), pb = u8_valid(tb, xmax_b, ymax_b);
            blend_frame<BYTES_A>(acc, im_a, lo_a, ta, pa, xmax_a, ymax_a, feather, g, o, 0u);
            blend_frame<BYTES_B>(acc, im_b, lo_b, tb, pb, xmax_b, ymax_b, feather, 1.0f, 0.0f, 1u);
#pragma unroll
            for (int c = 0; c < 3; ++c) q[p * 3 + c] = u8_round(acc.value(c));
            code[p] = (pa ? 1u : 0u) | (pb ? 2u : 0u);
            win[p] = acc.winner;
        }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        u8_store_pixels<PX>(out + at * 3, q);
        if (cover) u8_store_flags<PX>(cover + at, code, cover_vec);
        if (winner) u8_store_flags<PX>(winner + at, win, winner_vec);
    }
}

// ------------------------------------------------------------------------------------------------
// feather / first / last: the two walks once more, with the rule written into them
// ------------------------------------------------------------------------------------------------
// As a Rule (num[3], den, cnt and the run-time mode in a struct; the pair mapping B_OVER_A to last and A_OVER_B to first) these two compute
// the same bits but the compiler keeps the struct's fields as scalars where it keeps the bare arrays below as vectors, and on an MI355X
// bh_pano_u8 then took 130 to 139 us where this form takes 120, bh_mosaic_u8 271 to 287 us for 265.  So they stay
// as they were: the sequence walk with the accumulators as arrays over the thread's pixels, the pair walk with the closed form of n = 2.
// grid (pano_grid_x, u8_grid_y(B)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (count_vec: count % 4 == 0 too)
template <int PX, bool BYTES>
__global__ void __launch_bounds__(BLEND_THREADS) pano_kernel(const unsigned char* __restrict__ images, const int* __restrict__ idx, int n_images, int Hs, int Ws,
                                                            const double* __restrict__ M64, const double* __restrict__ gain, const unsigned char* __restrict__ use,
                                                            int B, int n, int Hc, int Wc, float feather, int mode,
                                                            unsigned char* __restrict__ out, unsigned char* __restrict__ count, int count_vec) {
#pragma clang fp contract(off)
    int x, y;
    if (!pano_unit<PX>(Hc, Wc, x, y)) return;
    const unsigned npix = (unsigned)Hs * (unsigned)Ws;
    const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        float num[PX * 3], den[PX];
        unsigned cnt[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) { num[p * 3] = num[p * 3 + 1] = num[p * 3 + 2] = den[p] = 0.0f; cnt[p] = 0u; }
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
#if PANO_SKIP
            if (!__any(any)) continue;                                         // absent from the whole wavefront: no load at all
#endif
            const float g = gain ? (float)gain[2 * f] : 1.0f, o = gain ? (float)gain[2 * f + 1] : 0.0f;
            const U8Image im = u8_image(images, idx ? idx + (size_t)b * n : nullptr, k, n_images, npix);
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const U8Sample s = u8_gather<BYTES>(im, t[p], xmax, ymax);
                const float w = u8_border_weight(s, xmax, ymax, feather);
                const bool first = cnt[p] == 0u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = __builtin_fmaf(g, s.c[c], o), wv = w * v, acc = num[p * 3 + c];
                    const float next = mode == BH_PANO_FEATHER ? acc + wv : ((mode == BH_PANO_LAST || first) ? v : acc);
                    num[p * 3 + c] = present[p] ? next : acc;
                }
                den[p] = present[p] ? den[p] + w : den[p];
                cnt[p] += present[p] ? 1u : 0u;
            }
        }
        unsigned q[PX * 3];
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = mode == BH_PANO_FEATHER ? (den[p] > 0.0f ? num[p * 3 + c] / den[p] : 0.0f) : num[p * 3 + c];
                q[p * 3 + c] = u8_round(v);
            }
        const size_t at = ((size_t)b * Hc + y) * Wc + x;
        u8_store_pixels<PX>(out + at * 3, q);
        if (count) u8_store_flags<PX>(count + at, cnt, count_vec);
    }
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

// grid (row_grid_x, u8_grid_y(B)); PX = 4: Wc % 4 == 0 and out % 4 == 0 (cover_vec: cover % 4 == 0 too)
template <int PX, bool BYTES_A, bool BYTES_B>
__global__ void __launch_bounds__(BLEND_THREADS) mosaic_kernel(const unsigned char* __restrict__ images_a, const int* __restrict__ idx_a, int n_a, int Ha, int Wa,
                                                                const unsigned char* __restrict__ images_b, const int* __restrict__ idx_b, int n_b, int Hb, int Wb,
                                                                const double* __restrict__ Ma64, const double* __restrict__ Mb64, const double* __restrict__ gain,
                                                                int B, int Hc, int Wc, float feather, int mode,
                                                                unsigned char* __restrict__ out, unsigned char* __restrict__ cover, int cover_vec) {
    int x, y;
    if (!row_unit<PX>(Hc, Wc, x, y)) return;
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

// ------------------------------------------------------------------------------------------------
// the launches, one per walk; the entry points add their own refusals and name their kernel
// ------------------------------------------------------------------------------------------------
static bool blend_bank_bad(const void* images, int n_images, int H, int W) { return !images || n_images < 1 || H < 1 || W < 1; }
// `bad`: the walk's own NULL pointers, banks and frame count.  BH_E_BADARG comes before BH_E_UNSUPPORTED for a call that breaks both;
// image_pixels: the larger image (tap_place's offsets are ints of 4 bytes per pixel, byte offsets inside an image 32-bit; the unit index
// of a thread is an unsigned)
static int blend_refuse(bool bad, int B, int Hc, int Wc, float feather, long long image_pixels) {
    if (bad || B < 0 || Hc < 1 || Wc < 1 || u8_feather_bad(feather)) return BH_E_BADARG;
    if (image_pixels > (1ll << 29) || (long long)Hc * Wc > 0x7fffffffll) return BH_E_UNSUPPORTED;
    return BH_OK;
}
static int blend_plane_vec(const void* plane) { return plane && reinterpret_cast<uintptr_t>(plane) % 4 == 0; }

// launch(four, bytes, grid, stream, flags_vec): four - a thread makes four pixels; bytes - a single-pixel frame, no room for 4-byte loads
template <class Launch>
static int blend_seq(const uint8_t* images, int n_images, int Hs, int Ws, const double* M, int B, int n, int Hc, int Wc, float feather, uint8_t* out,
                     uint8_t* count, void* stream, Launch&& launch) {
    const bool bad = blend_bank_bad(images, n_images, Hs, Ws) || !M || !out || n < 1 || n > BLEND_MAX_FRAMES;
    if (const int rc = blend_refuse(bad, B, Hc, Wc, feather, (long long)Hs * Ws)) return rc;
    if (B == 0) return BH_OK;
    const U8Stores stores = u8_stores(Wc, out, count);
    const dim3 grid(pano_grid_x(Hc, Wc, stores.vec ? 4 : 1), u8_grid_y(B));
    u8_flags([&](auto four, auto by) { launch(four, by, grid, bh_stream(stream), stores.flag_vec); }, stores.vec, (long long)Hs * Ws < 2);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

// launch(four, bytes_a, bytes_b, grid, stream, flags_vec)
template <class Launch>
static int blend_pair(const uint8_t* images_a, int n_a, int Ha, int Wa, const uint8_t* images_b, int n_b, int Hb, int Wb, const double* Ma, const double* Mb,
                      int B, int Hc, int Wc, float feather, uint8_t* out, uint8_t* cover, void* stream, Launch&& launch) {
    const bool bad = blend_bank_bad(images_a, n_a, Ha, Wa) || blend_bank_bad(images_b, n_b, Hb, Wb) || !Ma || !Mb || !out;
    const long long pa = (long long)Ha * Wa, pb = (long long)Hb * Wb;
    if (const int rc = blend_refuse(bad, B, Hc, Wc, feather, pa > pb ? pa : pb)) return rc;
    if (B == 0) return BH_OK;
    const U8Stores stores = u8_stores(Wc, out, cover);
    const dim3 grid(row_grid_x(Hc, Wc, stores.vec ? 4 : 1), u8_grid_y(B));
    u8_flags([&](auto four, auto by_a, auto by_b) { launch(four, by_a, by_b, grid, bh_stream(stream), stores.flag_vec); }, stores.vec, pa < 2, pb < 2);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

extern "C" {

int bh_pano_u8(const uint8_t* images, const int* idx, int n_images, int Hs, int Ws, const double* M, const double* gain,
               const uint8_t* use, int B, int n, int Hc, int Wc, float feather, int mode, uint8_t* out, uint8_t* count, void* stream) {
    if (mode != BH_PANO_FEATHER && mode != BH_PANO_FIRST && mode != BH_PANO_LAST) return BH_E_BADARG;
    return blend_seq(images, n_images, Hs, Ws, M, B, n, Hc, Wc, feather, out, count, stream, [&](auto four, auto by, dim3 grid, hipStream_t st, int count_vec) {
        hipLaunchKernelGGL((pano_kernel<four ? 4 : 1, by>), grid, dim3(BLEND_THREADS), 0, st, images, idx, n_images, Hs, Ws, M, gain, use, B, n, Hc, Wc, feather,
                           mode, out, count, count_vec);
    });
}

int bh_pano_bands_u8(const uint8_t* images, const uint8_t* low, const int* idx, int n_images, int Hs, int Ws, const double* M, const double* gain,
                     const uint8_t* use, int B, int n, int Hc, int Wc, float feather, uint8_t* out, uint8_t* count, uint8_t* winner, void* stream) {
    if (!low) return BH_E_BADARG;
    return blend_seq(images, n_images, Hs, Ws, M, B, n, Hc, Wc, feather, out, count, stream, [&](auto four, auto by, dim3 grid, hipStream_t st, int count_vec) {
        hipLaunchKernelGGL((blend_seq_kernel<BandRule, four ? 4 : 1, by>), grid, dim3(BLEND_THREADS), 0, st, images, low, idx, n_images, Hs, Ws, M, gain, use, B, n,
                           Hc, Wc, feather, out, count, winner, count_vec, blend_plane_vec(winner));
    });
}

int bh_mosaic_u8(const uint8_t* images_a, const int* idx_a, int n_a, int Ha, int Wa,
                 const uint8_t* images_b, const int* idx_b, int n_b, int Hb, int Wb,
                 const double* Ma, const double* Mb, const double* gain,
                 int B, int Hc, int Wc, float feather, int mode,
                 uint8_t* out, uint8_t* cover, void* stream) {
    if (mode != BH_MOSAIC_FEATHER && mode != BH_MOSAIC_B_OVER_A && mode != BH_MOSAIC_A_OVER_B) return BH_E_BADARG;
    return blend_pair(images_a, n_a, Ha, Wa, images_b, n_b, Hb, Wb, Ma, Mb, B, Hc, Wc, feather, out, cover, stream,
                      [&](auto four, auto by_a, auto by_b, dim3 grid, hipStream_t st, int cover_vec) {
        hipLaunchKernelGGL((mosaic_kernel<four ? 4 : 1, by_a, by_b>), grid, dim3(BLEND_THREADS), 0, st, images_a, idx_a, n_a, Ha, Wa, images_b, idx_b, n_b, Hb, Wb,
                           Ma, Mb, gain, B, Hc, Wc, feather, mode, out, cover, cover_vec);
    });
}

int bh_mosaic_bands_u8(const uint8_t* images_a, const uint8_t* low_a, const int* idx_a, int n_a, int Ha, int Wa,
                       const uint8_t* images_b, const uint8_t* low_b, const int* idx_b, int n_b, int Hb, int Wb,
                       const double* Ma, const double* Mb, const double* gain,
                       int B, int Hc, int Wc, float feather,
                       uint8_t* out, uint8_t* cover, uint8_t* winner, void* stream) {
    if (!low_a || !low_b) return BH_E_BADARG;
    return blend_pair(images_a, n_a, Ha, Wa, images_b, n_b, Hb, Wb, Ma, Mb, B, Hc, Wc, feather, out, cover, stream,
                      [&](auto four, auto by_a, auto by_b, dim3 grid, hipStream_t st, int cover_vec) {
        hipLaunchKernelGGL((blend_pair_kernel<BandRule, four ? 4 : 1, by_a, by_b>), grid, dim3(BLEND_THREADS), 0, st, images_a, low_a, idx_a, n_a, Ha, Wa, images_b,
                           low_b, idx_b, n_b, Hb, Wb, Ma, Mb, gain, B, Hc, Wc, feather, out, cover, winner, cover_vec, blend_plane_vec(winner));
    });
}

}  // extern "C"
