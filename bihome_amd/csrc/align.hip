// Image alignment: the two passes over the pixels around a trained model (include/bihome.h "Image alignment"; bihome_amd/align.py holds
// the numpy float64 statements prep_host / warp_u8_host the kernels are tested against).
//
// bh_align_prep_u8: uint8 interleaved RGB image (a region of it) -> the standardised P x P patch the model reads, as an exact area
// average.  One thread per output pixel, all channels: it walks the source rows of its interval and, inside a row, the run of pixels its
// interval covers (neighbouring lanes read neighbouring runs).  Interval ends in double (the same expressions as the host statement),
// the overlaps (relative to the first pixel of the run) and the sums in float.  A pixel is one 4-byte load of any alignment (u8_image.h
// ld_rgb_u8).
//
// bh_warp_u8: out(x, y) = bilinear image(H (x, y, 1)) on interleaved uint8, zero padding, round half up, with the validity mask: the
// sample, its `valid` and the stores are u8_image.h's (u8_sample, u8_round, u8_store_pixels / u8_store_flags).  Wo % 4 == 0 and out on a
// 4-byte boundary: a thread makes four pixels and stores three dwords; anything else: one pixel, three byte stores.
//
// The offset of an image in the bank is 64-bit (image 9,321 of a 240 x 320 bank starts past 2^31 bytes; inside an image offsets are
// 32-bit), the image index is clamped, and every source pixel index is clamped to its image (u8_image.h u8_image).  No atomics, no
// scratch, one writer per output element.
#include "u8_image.h"

#define ALIGN_THREADS 256

// floor / ceil results as indices inside [0, n - 1], whatever the double is (NaN -> 0)
__device__ __forceinline__ int align_index(double f, int n) { return (int)fmin(fmax(f, 0.0), (double)(n - 1)); }

struct PrepGeom { double x0, y0, sx, sy; };

// per_p = 1 / P from the host: every thread needs sx and sy, and a double division is some forty instructions.  For a P that is no power
// of two rw * (1 / P) may differ from rw / P in the last bit - a 1e-16 shift of the cell edges; the geometry RECORD is divided (prep_record).
__device__ __forceinline__ PrepGeom prep_geom(const double* __restrict__ roi, int b, int H, int W, double per_p) {
#pragma clang fp contract(off)
    PrepGeom g;
    g.x0 = roi ? roi[4 * b] : 0.0;
    g.y0 = roi ? roi[4 * b + 1] : 0.0;
    g.sx = (roi ? roi[4 * b + 2] : (double)W) * per_p;
    g.sy = (roi ? roi[4 * b + 3] : (double)H) * per_p;
    return g;
}

// geom[b] = (sx, sy, tx, ty): the expressions of bihome_amd.align.prep_host, in its order and without contraction - the same bits
__device__ __forceinline__ void prep_record(const double* __restrict__ roi, int b, int H, int W, int P, double* __restrict__ gb) {
#pragma clang fp contract(off)
    const double x0 = roi ? roi[4 * b] : 0.0, y0 = roi ? roi[4 * b + 1] : 0.0;
    const double sx = (roi ? roi[4 * b + 2] : (double)W) / (double)P, sy = (roi ? roi[4 * b + 3] : (double)H) / (double)P;
    gb[0] = sx; gb[1] = sy;
    gb[2] = x0 + 0.5 * sx - 0.5;
    gb[3] = y0 + 0.5 * sy - 0.5;
}

// the interval [lo, hi) of output position k along one axis: lo = origin + k s, hi = origin + (k + 1) s
__device__ __forceinline__ void prep_interval(double origin, double s, int k, double& lo, double& hi) {
#pragma clang fp contract(off)
    lo = origin + (double)k * s;
    hi = origin + (double)(k + 1) * s;
}

// length of the overlap of [lo, hi) with the unit interval [k, k + 1), all relative to the first pixel of the run (float: small numbers)
__device__ __forceinline__ float prep_overlap(float lo, float hi, int k) {
    return fmaxf(fminf(hi, (float)(k + 1)) - fmaxf(lo, (float)k), 0.0f);
}

// grid (ceil(P * P / ALIGN_THREADS), u8_grid_y(B)); H * W <= 2^30
template <int C, bool BYTES>
__global__ void __launch_bounds__(ALIGN_THREADS) align_prep_kernel(const unsigned char* __restrict__ images, const int* __restrict__ idx, int n_images,
                                                                   int H, int W, const double* __restrict__ roi, int B, int P, double per_p,
                                                                   float mean, float std, float* __restrict__ patch, double* __restrict__ geom) {
    const unsigned u = blockIdx.x * ALIGN_THREADS + threadIdx.x;
    if (u >= (unsigned)(P * P)) return;
    const int y = (int)(u / (unsigned)P), x = (int)(u - (unsigned)y * (unsigned)P);
    const unsigned n = (unsigned)H * (unsigned)W;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const PrepGeom g = prep_geom(roi, b, H, W, per_p);
        if (u == 0) prep_record(roi, b, H, W, P, geom + 4 * (size_t)b);
        double xl, xh, yl, yh;
        prep_interval(g.x0, g.sx, x, xl, xh);
        prep_interval(g.y0, g.sy, y, yl, yh);
        const int i0 = align_index(floor(xl), W), i1 = align_index(ceil(xh) - 1.0, W);
        const int j0 = align_index(floor(yl), H), j1 = align_index(ceil(yh) - 1.0, H);
        // the interval relative to the first pixel of the run: the per-pixel overlaps are float arithmetic on small numbers
        const float fxl = (float)(xl - (double)i0), fxh = (float)(xh - (double)i0), fyl = (float)(yl - (double)j0), fyh = (float)(yh - (double)j0);
        const U8Image im = u8_image(images, idx, b, n_images, n);
        float ar = 0.f, ag = 0.f, ab = 0.f;
        for (int j = j0; j <= j1; ++j) {
            const unsigned row = (unsigned)j * (unsigned)W;
            float rr = 0.f, rg = 0.f, rb = 0.f;
            for (int i = i0; i <= i1; ++i) {
                const unsigned v = ld_rgb_u8<BYTES>(im, row + (unsigned)i);
                const float wx = prep_overlap(fxl, fxh, i - i0);
                rr = __builtin_fmaf(wx, (float)(v & 255u), rr);
                rg = __builtin_fmaf(wx, (float)((v >> 8) & 255u), rg);
                rb = __builtin_fmaf(wx, (float)((v >> 16) & 255u), rb);
            }
            const float wy = prep_overlap(fyl, fyh, j - j0);
            ar = __builtin_fmaf(wy, rr, ar);
            ag = __builtin_fmaf(wy, rg, ag);
            ab = __builtin_fmaf(wy, rb, ab);
        }
        const float inv = 1.0f / ((float)g.sx * (float)g.sy * 255.0f);
        u8_store_patch<C>(patch + (size_t)b * C * P * P + u, (size_t)P * P, ar, ag, ab, inv, mean, std);
    }
}

// grid (ceil(Ho * (Wo / PX) / ALIGN_THREADS), u8_grid_y(B)); PX = 4: Wo % 4 == 0 and out % 4 == 0 (valid_vec: valid % 4 == 0 too).
// The four-pixel form is a gather whose time is the latency of its sixteen loads: with five waves per SIMD as the target the compiler
// keeps eight of them in flight (77-81 registers), with the default of eight it takes 52 registers, waits for every load before it
// issues the next and 64 pairs of 480 x 640 take 80 us instead of 66.
template <int PX, bool BYTES>
__global__ void __launch_bounds__(ALIGN_THREADS) __attribute__((amdgpu_waves_per_eu(1, PX == 4 ? 5 : 8)))
align_warp_kernel(const unsigned char* __restrict__ images, const int* __restrict__ idx, int n_images, int Hs, int Ws, const double* __restrict__ H64,
                  int B, int Ho, int Wo, unsigned char* __restrict__ out, unsigned char* __restrict__ valid, int valid_vec) {
    const unsigned upr = (unsigned)Wo / PX;                                    // units per output row
    const unsigned u = blockIdx.x * ALIGN_THREADS + threadIdx.x;
    if (u >= upr * (unsigned)Ho) return;
    const int y = (int)(u / upr), x = (int)(u - (unsigned)y * upr) * PX;
    const unsigned n = (unsigned)Hs * (unsigned)Ws;
    const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Hf Hm = load_h(H64 + 9 * (size_t)b);
        const U8Image im = u8_image(images, idx, b, n_images, n);
        unsigned o[PX * 3], ok[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const U8Sample s = u8_sample<BYTES>(im, Hm, x + p, y, Ws, Hs, xmax, ymax);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[p * 3 + c] = u8_round(s.c[c]);
            ok[p] = s.valid ? 1u : 0u;
        }
        const size_t at = ((size_t)b * Ho + y) * Wo + x;
        u8_store_pixels<PX>(out + at * 3, o);
        if (valid) u8_store_flags<PX>(valid + at, ok, valid_vec);
    }
}

// what both entry points refuse as BH_E_BADARG apart from their NULL pointers: a negative batch or a bank / image without extent
static bool align_extents_bad(int count, int n_images, int h, int w) { return count < 0 || n_images < 1 || h < 1 || w < 1; }

extern "C" {

int bh_align_prep_u8(const uint8_t* images, const int* idx, int n_images, int H, int W, const double* roi,
                     int B, int P, int C, float mean, float std, float* patch, double* geom, void* stream) {
    if (!images || !patch || !geom || align_extents_bad(B, n_images, H, W) || P < 1 || !(std != 0.0f) || std != std) return BH_E_BADARG;
    if ((C != 1 && C != 3) || P % 16 != 0 || P > 256 || (long long)H * W > (1ll << 30)) return BH_E_UNSUPPORTED;      // (32-bit offsets inside an image)
    if (B == 0) return BH_OK;
    const dim3 grid((unsigned)(P * P + ALIGN_THREADS - 1) / ALIGN_THREADS, u8_grid_y(B));
    hipStream_t st = bh_stream(stream);
    const bool bytes = (long long)H * W < 2;                                    // a single-pixel image: no room for 4-byte loads
    u8_flags([&](auto gray, auto by) {
        hipLaunchKernelGGL((align_prep_kernel<gray ? 1 : 3, by>), grid, dim3(ALIGN_THREADS), 0, st, images, idx, n_images, H, W, roi, B, P, 1.0 / (double)P, mean, std, patch, geom);
    }, C == 1, bytes);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_warp_u8(const uint8_t* images, const int* idx, int n_images, int Hs, int Ws, const double* H64,
               int B, int Ho, int Wo, uint8_t* out, uint8_t* valid, void* stream) {
    if (!images || !H64 || !out || align_extents_bad(B, n_images, Hs, Ws) || Ho < 1 || Wo < 1) return BH_E_BADARG;
    // (tap_place's offsets are ints of 4 bytes per pixel, byte offsets inside an image 32-bit; the unit index of a thread is an unsigned)
    if ((long long)Hs * Ws > (1ll << 29) || (long long)Ho * Wo > 0x7fffffffll) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const bool vec = Wo % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const int valid_vec = valid && reinterpret_cast<uintptr_t>(valid) % 4 == 0;
    const unsigned units = (unsigned)Ho * ((unsigned)Wo / (vec ? 4 : 1));
    const dim3 grid((units + ALIGN_THREADS - 1) / ALIGN_THREADS, u8_grid_y(B));
    hipStream_t st = bh_stream(stream);
    const bool bytes = (long long)Hs * Ws < 2;                                  // a single-pixel image: no room for 4-byte loads
    u8_flags([&](auto four, auto by) {
        hipLaunchKernelGGL((align_warp_kernel<four ? 4 : 1, by>), grid, dim3(ALIGN_THREADS), 0, st, images, idx, n_images, Hs, Ws, H64, B, Ho, Wo, out, valid, valid_vec);
    }, vec, bytes);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
