// The low band of the two-band blend: a Gaussian low-pass of uint8 RGB bank images in integer arithmetic (include/bihome.h "Two-band
// blend"; bihome_amd/align.py holds the numpy statements blur_taps / blur_host the kernel equals bit for bit).
//
// bh_blur_u8: L[y,x,c] = (sum_j sum_i w|j| w|i| I[clamp(y + j), clamp(x + i), c] + 2^21) >> 22 with integer taps that sum to 2048, so the
// sum is exact in 32-bit unsigned words (255 * 2048 * 2048 < 2^31) and its order does not show.  One launch for all samples, one
// workgroup per BLUR_TW x BLUR_TH tile of the image, separable through LDS:
//   1. the tile's bytes with its halo, border replicated (every coordinate clamped), one pixel per thread and round (u8_image.h's
//      ld_rgb_u8: one 4-byte load of any alignment) - the halo is `radius` rows above and below and `radius` rounded up to a multiple of
//      four pixels on either side, so that every thread of step 2 starts on a dword;
//   2. rows: a thread makes 4 consecutive pixels x 3 channels of one staged row from (4 + 2 RH) pixels read as dwords - 3 dwords per 4
//      pixels instead of 12 byte reads - into 32-bit LDS words;
//   3. columns: a thread makes 4 consecutive rows of one column-channel from 4 + 2 radius words (consecutive lanes on consecutive
//      words), rounds and stores bytes.
// The taps travel by value in the kernel-argument struct, padded with zeros up to the largest distance step 2 can ask for: every tap
// index is the same for the whole wavefront and no tap needs a bound check.  No atomics, one writer per output byte.
#include "u8_image.h"

#define BLUR_THREADS 256
#define BLUR_TW 32                 // the tile: pixels per row (a multiple of 4)
#define BLUR_TH 24                 // ... and rows (a multiple of 4); with radius 32 the two LDS arrays take 59,136 bytes
#define BLUR_MAX_RADIUS 32
#define BLUR_TAPS (BLUR_MAX_RADIUS + 4)        // |distance| <= radius + 3 in the 4-wide units of both passes

struct BlurTaps { int w[BLUR_TAPS]; };         // w[d] for d <= radius, 0 beyond

static inline int blur_halo_x(int radius) { return (radius + 3) & ~3; }
static inline unsigned blur_stage_row_bytes(int radius) { return (unsigned)(BLUR_TW + 2 * blur_halo_x(radius)) * 3u; }      // (a multiple of 12)
static inline unsigned blur_rows(int radius) { return (unsigned)(BLUR_TH + 2 * radius); }
static inline size_t blur_lds_bytes(int radius) {
    return (size_t)blur_rows(radius) * blur_stage_row_bytes(radius) + (size_t)blur_rows(radius) * (BLUR_TW * 3) * sizeof(unsigned);
}

// grid (tiles_x * tiles_y, u8_grid_y(count)); dynamic LDS blur_lds_bytes(radius): the row sums first (16-byte aligned), then the bytes
template <bool BYTES>
__global__ void __launch_bounds__(BLUR_THREADS) blur_kernel(const unsigned char* __restrict__ images, const int* __restrict__ idx, int n_images, int H, int W,
                                                            int count, const BlurTaps taps, int radius, unsigned char* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char blur_lds[];
    const int RH = (radius + 3) & ~3;
    const int rows = BLUR_TH + 2 * radius, stage_px = BLUR_TW + 2 * RH;
    const unsigned row_bytes = (unsigned)stage_px * 3u;
    unsigned* __restrict__ hsum = reinterpret_cast<unsigned*>(blur_lds);                            // [rows][BLUR_TW * 3]
    unsigned char* __restrict__ stage = blur_lds + (size_t)rows * (BLUR_TW * 3) * sizeof(unsigned);  // [rows][stage_px * 3]
    const unsigned tiles_x = ((unsigned)W + BLUR_TW - 1) / BLUR_TW, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = (int)tx * BLUR_TW, y0 = (int)ty * BLUR_TH;
    const unsigned npix = (unsigned)H * (unsigned)W;
    for (int s = blockIdx.y; s < count; s += gridDim.y) {
        const U8Image im = u8_image(images, idx, s, n_images, npix);
        // 1. the bytes, border replicated
        for (int i = threadIdx.x; i < rows * stage_px; i += BLUR_THREADS) {
            const int r = i / stage_px, c = i - r * stage_px;
            int y = y0 - radius + r, x = x0 - RH + c;
            y = y < 0 ? 0 : (y >= H ? H - 1 : y);
            x = x < 0 ? 0 : (x >= W ? W - 1 : x);
            const unsigned p = ld_rgb_u8<BYTES>(im, (unsigned)y * (unsigned)W + (unsigned)x);
            unsigned char* d = stage + (unsigned)r * row_bytes + 3u * (unsigned)c;
            d[0] = (unsigned char)p; d[1] = (unsigned char)(p >> 8); d[2] = (unsigned char)(p >> 16);
        }
        __syncthreads();
        // 2. rows: unit u = (staged row, group of 4 pixels)
        for (int u = threadIdx.x; u < rows * (BLUR_TW / 4); u += BLUR_THREADS) {
            const int r = u / (BLUR_TW / 4), g = u - r * (BLUR_TW / 4);
            const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(stage + (unsigned)r * row_bytes + 12u * (unsigned)g);      // pixel 4 g of the staged row
            unsigned acc[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[k] = 0u;
            // output o (0..3) is staged pixel 4 g + RH + o; input pixel 4 q + j of the window sits at distance 4 q + j - RH - o
            for (int q = 0; q < 1 + RH / 2; ++q) {
                const unsigned d0 = src[3 * q], d1 = src[3 * q + 1], d2 = src[3 * q + 2];
                const unsigned px[12] = {d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u, d0 >> 24, d1 & 255u, (d1 >> 8) & 255u,
                                         (d1 >> 16) & 255u, d1 >> 24, d2 & 255u, (d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24};
                const int base = 4 * q - RH;
                unsigned tw[7];                                                // the taps at distances base - 3 .. base + 3
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    int d = base - 3 + k;
                    d = d < 0 ? -d : d;
                    tw[k] = d < BLUR_TAPS ? (unsigned)taps.w[d] : 0u;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int o = 0; o < 4; ++o)
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[o * 3 + c] += tw[j - o + 3] * px[j * 3 + c];
            }
            unsigned* __restrict__ dst = hsum + (unsigned)r * (BLUR_TW * 3) + 12u * (unsigned)g;
#pragma unroll
            for (int k = 0; k < 12; ++k) dst[k] = acc[k];
        }
        __syncthreads();
        // 3. columns: unit u = (group of 4 rows, column-channel)
        unsigned char* __restrict__ o_img = out + (size_t)s * npix * 3u;
        for (int u = threadIdx.x; u < (BLUR_TH / 4) * (BLUR_TW * 3); u += BLUR_THREADS) {
            const int rg = u / (BLUR_TW * 3), xc = u - rg * (BLUR_TW * 3);
            const unsigned* __restrict__ src = hsum + (unsigned)(4 * rg) * (BLUR_TW * 3) + (unsigned)xc;      // staged row 4 rg: distance -radius of output 0
            unsigned acc[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < 4 + 2 * radius; ++j) {
                const unsigned v = src[(unsigned)j * (BLUR_TW * 3)];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    int d = j - radius - o;
                    d = d < 0 ? -d : d;
                    acc[o] += (d < BLUR_TAPS ? (unsigned)taps.w[d] : 0u) * v;
                }
            }
            const int x = x0 + xc / 3;
            if (x < W) {
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int y = y0 + 4 * rg + o;
                    if (y < H) o_img[((size_t)y * W + x) * 3u + (unsigned)(xc % 3)] = (unsigned char)((acc[o] + (1u << 21)) >> 22);
                }
            }
        }
        __syncthreads();                                                       // (the next sample stages over what step 3 read)
    }
}

// the taps an entry refuses: a radius outside 1..32, a negative tap, taps[0] + 2 sum_{i >= 1} taps[i] != 2048
static bool blur_taps_bad(const int* taps, int radius) {
    if (radius < 1 || radius > BLUR_MAX_RADIUS) return true;
    long long sum = 0;
    for (int i = 0; i <= radius; ++i) {
        if (taps[i] < 0) return true;
        sum += (i ? 2ll : 1ll) * taps[i];
    }
    return sum != 2048;
}

extern "C" {

int bh_blur_u8(const uint8_t* images, const int* idx, int n_images, int H, int W, int count, const int* taps, int radius, uint8_t* out,
               void* stream) {
    if (!images || !taps || !out || count < 0 || n_images < 1 || H < 1 || W < 1 || blur_taps_bad(taps, radius)) return BH_E_BADARG;
    // (ld_rgb_u8's byte offsets inside an image are 32-bit)
    if ((long long)H * W > (1ll << 29)) return BH_E_UNSUPPORTED;
    if (count == 0) return BH_OK;
    BlurTaps t;
    for (int i = 0; i < BLUR_TAPS; ++i) t.w[i] = i <= radius ? taps[i] : 0;
    const unsigned tiles = (((unsigned)W + BLUR_TW - 1) / BLUR_TW) * (((unsigned)H + BLUR_TH - 1) / BLUR_TH);
    const dim3 grid(tiles, u8_grid_y(count));
    hipStream_t st = bh_stream(stream);
    const bool bytes = (long long)H * W < 2;                                   // a single-pixel image: no room for 4-byte loads
    u8_flags([&](auto by) {
        hipLaunchKernelGGL((blur_kernel<by>), grid, dim3(BLUR_THREADS), blur_lds_bytes(radius), st, images, idx, n_images, H, W, count, t, radius, out);
    }, bytes);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
