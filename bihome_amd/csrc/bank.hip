// Resident image bank of the pair generator: what the reference's Dataset.load_image (src/data/coco/dataset.py:95-103) does on the host,
// one np.load of a uint8 [H,W,3] RGB array per sample, is here a gather out of ONE uint8 tensor bank[n_images,Hs,Ws,3] that stays in HBM
// (COCO train2014 after preprocess_offline.py: 82,783 x 240 x 320 x 3 bytes = 19 GB).  A batch's images leave it as the float planes
// [count,3,Hs,Ws], values 0..255, that bh_synth_batch / bh_synth_image already read: the generator's arithmetic stays where it is.
//
// An image is Hs*Ws pixels in a row both in the bank (interleaved) and in each output plane, so the kernels see it flat.  Vector path
// (Hs*Ws % 4 == 0 - every Ws % 4 == 0 - and bank / out on 4 / 16-byte boundaries): a thread takes four pixels = three dwords (one
// 12-byte load, consecutive lanes on consecutive 12 bytes) and stores one float4 into each of the three planes (consecutive lanes on
// consecutive 16 bytes).  Scalar path (anything else): a thread takes one pixel, three byte loads and three float stores.  Every byte
// offset is 64-bit: image 9,321 of a 240 x 320 bank already starts past 2^31.  No atomics, every output element written exactly once.
// Which image a sample reads (an index outside [0, n_images) is clamped into it), the 12-byte struct and the pixel store are u8_image.h's.
#include "u8_image.h"

#define BANK_THREADS 256

// grid (ceil(n/4 / BANK_THREADS), u8_grid_y(count)), n = Hs*Ws pixels per image, n % 4 == 0
__global__ void __launch_bounds__(BANK_THREADS) bank_gather_vec4_kernel(const unsigned char* __restrict__ bank, const int* __restrict__ img_idx,
                                                                        int count, int n_images, size_t n, float* __restrict__ out) {
    const size_t u = (size_t)blockIdx.x * BANK_THREADS + threadIdx.x;          // unit = pixels 4u .. 4u+3
    if (u >= n / 4) return;
    for (int b = blockIdx.y; b < count; b += gridDim.y) {
        const unsigned char* src = bank + u8_image_index(img_idx, b, n_images) * n * 3;
        const Dwords3 d = reinterpret_cast<const Dwords3*>(src)[u];
        // bytes, lowest first: d.a = r0 g0 b0 r1, d.b = g1 b1 r2 g2, d.c = b2 r3 g3 b3
        const float4 r = make_float4((float)(d.a & 255u), (float)(d.a >> 24), (float)((d.b >> 16) & 255u), (float)((d.c >> 8) & 255u));
        const float4 g = make_float4((float)((d.a >> 8) & 255u), (float)(d.b & 255u), (float)(d.b >> 24), (float)((d.c >> 16) & 255u));
        const float4 bl = make_float4((float)((d.a >> 16) & 255u), (float)((d.b >> 8) & 255u), (float)(d.c & 255u), (float)(d.c >> 24));
        float* dst = out + (size_t)b * 3 * n + u * 4;
        *reinterpret_cast<float4*>(dst) = r;
        *reinterpret_cast<float4*>(dst + n) = g;
        *reinterpret_cast<float4*>(dst + 2 * n) = bl;
    }
}

// grid (ceil(n / BANK_THREADS), u8_grid_y(count)): any n, any alignment
__global__ void __launch_bounds__(BANK_THREADS) bank_gather_scalar_kernel(const unsigned char* __restrict__ bank, const int* __restrict__ img_idx,
                                                                          int count, int n_images, size_t n, float* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * BANK_THREADS + threadIdx.x;
    if (p >= n) return;
    for (int b = blockIdx.y; b < count; b += gridDim.y) {
        const unsigned char* src = bank + (u8_image_index(img_idx, b, n_images) * n + p) * 3;
        float* dst = out + (size_t)b * 3 * n + p;
        dst[0] = (float)src[0];
        dst[n] = (float)src[1];
        dst[2 * n] = (float)src[2];
    }
}

// ---- ingest: raw-size images into bank slots ------------------------------------------------------------------------------------------
// Upstream's Rescale((W, H)) + CenterCrop((W, H)) (src/data/transforms.py:24-46, 103-122; preprocess_offline.py runs them through
// cv2.resize one image at a time on the host) for `count` interleaved RGB uint8 images of DIFFERENT sizes in one launch: image b lies at
// src + src_off[b] with src_hw[b] = (h, w) and lands in slot first + b.  The resized image is never stored: a thread computes output
// pixels (y, x) = resized pixels (y + top, x + left) only.  Per image (every thread restates it, nothing goes through HBM):
//   r = h / w (double); r < H / W: (nw, nh) = (rint(H / r), H), else (W, rint(W r)); top = (nh - H) / 2, left = (nw - W) / 2.
// The resize is cv2.resize's default (INTER_LINEAR on 8-bit data) AS RECALLED, not read from OpenCV's source:
//   w == 2 nw and h == 2 nh: the rounded mean of the 2x2 block, (s00 + s01 + s10 + s11 + 2) >> 2;  (nh, nw) == (h, w): a copy;
//   otherwise two taps per axis, f = (float)((d + 0.5) * (n / n_new) - 0.5) (the product and the difference in double, NOT contracted),
//   s = floor(f), f -= s, clamped to [0, n - 1] with f = 0 at either end, coefficients rint((1 - f) 2048) and rint(f 2048) (float,
//   half to even), S = s[sx] a0 + s[sx + 1] a1 per row in int32 and out = (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.
// bihome_amd/bank.py rescale_center_crop_host is the numpy statement the kernel is held to bit for bit.
// Threads run along the output row and on into the next one.  W % 4 == 0 with the bank on a 4-byte boundary: a thread takes four pixels
// and stores three dwords (consecutive lanes on consecutive 12 bytes); anything else: one pixel, three byte stores.  The source side has
// no alignment to rely on (src_off is any byte, a row is 3 w bytes): its loads are written for any alignment, contiguous runs in the
// halving and copy paths (the compiler merges them), the two taps of a row as six bytes in the fixed-point path.  Every offset is 64-bit.  A source with h < 1 or w < 1
// (or whose resized size does not fit an int) leaves its slot untouched.  No atomics, no scratch, every output byte written once.
#define INGEST_SKIP 0
#define INGEST_FIXED 1
#define INGEST_HALVE 2
#define INGEST_COPY 3

struct IngestGeom { int h, w, top, left, mode; double sx, sy; };
struct IngestTap { int i0, i1, c0, c1; };          // the two source indices (i1 == i0 at the far edge) and their 11-bit coefficients

__device__ __forceinline__ IngestGeom ingest_geom(const int* __restrict__ src_hw, int b, int H, int W) {
#pragma clang fp contract(off)
    IngestGeom g;
    g.h = src_hw[2 * b]; g.w = src_hw[2 * b + 1];
    g.top = g.left = 0; g.sx = g.sy = 1.0; g.mode = INGEST_SKIP;
    if (g.h < 1 || g.w < 1) return g;
    const double r = (double)g.h / (double)g.w;
    double nwd = (double)W, nhd = (double)H;
    if (r < (double)H / (double)W) nwd = rint((double)H / r); else nhd = rint((double)W * r);
    if (!(nwd >= (double)W && nhd >= (double)H && nwd < 2147483648.0 && nhd < 2147483648.0)) return g;
    const int nw = (int)nwd, nh = (int)nhd;
    g.top = (nh - H) / 2; g.left = (nw - W) / 2;
    g.sx = (double)g.w / nwd; g.sy = (double)g.h / nhd;
    g.mode = ((long long)g.w == 2ll * nw && (long long)g.h == 2ll * nh) ? INGEST_HALVE : ((nw == g.w && nh == g.h) ? INGEST_COPY : INGEST_FIXED);
    return g;
}

// d: position in the resized image, scale = n / n_new, n: source extent.  Both indices lie in [0, n - 1] whatever d and scale are.
__device__ __forceinline__ IngestTap ingest_tap(int d, double scale, int n) {
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    int s = fl < 0.f ? -1 : (fl < 2147483520.f ? (int)fl : 0x7fffffff);
    f -= fl;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    IngestTap t;
    t.i0 = s; t.i1 = s + 1 < n ? s + 1 : s;
    t.c0 = (int)rintf((1.f - f) * 2048.f); t.c1 = (int)rintf(f * 2048.f);
    return t;
}

// The pixels of the two taps t of one source row as bytes 0..2 and 3..5 of the result.  The taps are neighbours (i1 == i0 + 1) everywhere
// but at the far edge, where i1 == i0 = w - 1 and the second coefficient is 0: there the six bytes read are pixels w - 2 and w - 1 and
// the first tap is moved down (the second reads as 0, times 0).  So one 4-byte and one 2-byte read, of any alignment, inside the row
// in every case; a single-column source (w == 1) has three bytes per row.  Per-byte reads cost three times the memory instructions.
__device__ __forceinline__ unsigned long long ingest_taps6(const unsigned char* __restrict__ row, const IngestTap& t, int w) {
    if (w < 2) return (unsigned long long)(row[0] | (row[1] << 8) | (row[2] << 16));
    const bool edge = t.i1 == t.i0;
    const unsigned char* p = row + (size_t)(edge ? t.i0 - 1 : t.i0) * 3;
    unsigned lo;
    unsigned short hi;
    __builtin_memcpy(&lo, p, 4);
    __builtin_memcpy(&hi, p + 4, 2);
    const unsigned long long v = lo | ((unsigned long long)hi << 32);
    return edge ? v >> 24 : v;
}

// grid (ceil(H * (W / PX) / BANK_THREADS), u8_grid_y(count)); PX = 4: W % 4 == 0 and bank % 4 == 0; H * W < 2^31
template <int PX>
__global__ void __launch_bounds__(BANK_THREADS) bank_ingest_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ src_off,
                                                                   const int* __restrict__ src_hw, int count, unsigned char* __restrict__ bank,
                                                                   int first, int H, int W) {
    const unsigned upr = (unsigned)W / PX;                                     // units per output row
    const unsigned u = blockIdx.x * BANK_THREADS + threadIdx.x;
    if (u >= upr * (unsigned)H) return;
    const int y = (int)(u / upr), x = (int)(u - (unsigned)y * upr) * PX;
    for (int b = blockIdx.y; b < count; b += gridDim.y) {
        const IngestGeom g = ingest_geom(src_hw, b, H, W);
        if (g.mode == INGEST_SKIP) continue;
        const unsigned char* s = src + src_off[b];
        const size_t pitch = (size_t)g.w * 3;
        const int dy = y + g.top, dx = x + g.left;                             // < nh, < nw: inside the resized image
        unsigned o[PX * 3];
        if (g.mode == INGEST_FIXED) {
            const IngestTap ty = ingest_tap(dy, g.sy, g.h);
            const unsigned char* r0 = s + (size_t)ty.i0 * pitch;
            const unsigned char* r1 = s + (size_t)ty.i1 * pitch;
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const IngestTap tx = ingest_tap(dx + p, g.sx, g.w);
                const unsigned long long v0 = ingest_taps6(r0, tx, g.w), v1 = ingest_taps6(r1, tx, g.w);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int S0 = (int)((v0 >> (8 * c)) & 255u) * tx.c0 + (int)((v0 >> (24 + 8 * c)) & 255u) * tx.c1;
                    const int S1 = (int)((v1 >> (8 * c)) & 255u) * tx.c0 + (int)((v1 >> (24 + 8 * c)) & 255u) * tx.c1;
                    o[p * 3 + c] = (unsigned)((((ty.c0 * (S0 >> 4)) >> 16) + ((ty.c1 * (S1 >> 4)) >> 16) + 2) >> 2);
                }
            }
        } else if (g.mode == INGEST_HALVE) {                                   // source pixels (2 dy .. 2 dy + 1, 2 dx .. 2 dx + 2 PX - 1)
            const unsigned char* r0 = s + (size_t)(2 * dy) * pitch + (size_t)(2 * dx) * 3;
            const unsigned char* r1 = r0 + pitch;
#pragma unroll
            for (int p = 0; p < PX; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    o[p * 3 + c] = ((unsigned)r0[p * 6 + c] + r0[p * 6 + 3 + c] + r1[p * 6 + c] + r1[p * 6 + 3 + c] + 2u) >> 2;
        } else {
            const unsigned char* r0 = s + (size_t)dy * pitch + (size_t)dx * 3;
#pragma unroll
            for (int i = 0; i < PX * 3; ++i) o[i] = r0[i];
        }
        u8_store_pixels<PX>(bank + (((size_t)(first + b) * H + y) * W + x) * 3, o);
    }
}

extern "C" {

int bh_bank_ingest_u8(const unsigned char* src, const int64_t* src_off, const int* src_hw, int count, unsigned char* bank, int n_slots,
                      int first, int H, int W, void* stream) {
    if (!src || !src_off || !src_hw || !bank || count < 0 || n_slots < 1 || H < 1 || W < 1 || first < 0 ||
        (long long)first + count > (long long)n_slots) return BH_E_BADARG;
    if (count == 0) return BH_OK;
    if ((long long)H * W > 0x7fffffffll) return BH_E_UNSUPPORTED;              // (more than 2^31 - 1 pixels in one bank image)
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(bank) % 4 == 0;
    const unsigned units = (unsigned)H * ((unsigned)W / (vec ? 4 : 1));
    const dim3 grid((units + BANK_THREADS - 1) / BANK_THREADS, u8_grid_y(count));
    hipStream_t st = bh_stream(stream);
    if (vec) hipLaunchKernelGGL(bank_ingest_kernel<4>, grid, dim3(BANK_THREADS), 0, st, src, src_off, src_hw, count, bank, first, H, W);
    else hipLaunchKernelGGL(bank_ingest_kernel<1>, grid, dim3(BANK_THREADS), 0, st, src, src_off, src_hw, count, bank, first, H, W);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_bank_gather_u8(const unsigned char* bank, const int* img_idx, int count, int n_images, int Hs, int Ws, float* out, void* stream) {
    if (!bank || !img_idx || !out || count < 0 || n_images < 1 || Hs < 1 || Ws < 1) return BH_E_BADARG;
    if (count == 0) return BH_OK;
    const size_t n = (size_t)Hs * Ws;
    const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(bank) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const size_t units = vec ? n / 4 : n;
    const size_t gx = (units + BANK_THREADS - 1) / BANK_THREADS;
    if (gx > 0x7fffffffull) return BH_E_UNSUPPORTED;                         // (more than 2^39 pixels in one image)
    const dim3 grid((unsigned)gx, u8_grid_y(count));
    hipStream_t st = bh_stream(stream);
    if (vec) hipLaunchKernelGGL(bank_gather_vec4_kernel, grid, dim3(BANK_THREADS), 0, st, bank, img_idx, count, n_images, n, out);
    else hipLaunchKernelGGL(bank_gather_scalar_kernel, grid, dim3(BANK_THREADS), 0, st, bank, img_idx, count, n_images, n, out);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
