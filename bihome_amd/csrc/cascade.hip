// Cascaded re-prediction: the two passes a stage of the cascade adds around the model (include/bihome.h "Cascaded re-prediction";
// bihome_amd/align.py holds the numpy float64 statements prep_warp_host / patch_ncc_host the kernels are tested against).
//
// bh_align_prep_warp_u8: image A seen through a homography, as the standardised P x P patch the model reads, without a full-size
// intermediate image.  One thread per patch pixel: it walks the ny x nx sub-sample points of its cell on a virtual integer grid of
// P ny x P nx points, each one bh_warp_u8's bilinear sample with its `valid` (u8_image.h u8_sample), and writes their mean
// (u8_store_patch) and the share of them that is valid.  The sub-samples are taken four at a time without a branch between them, so a thread has
// sixteen independent pixel loads in flight (a gather: neighbouring lanes read neighbouring cells, nothing coalesces beyond a cache
// line); what is left of nx ny after the groups of four is taken one by one.  Sums are float, in the fixed order of the walk.
//
// bh_patch_ncc: the zero-mean normalised correlation of two patches over the fully covered pixels.  One workgroup per sample, double
// accumulators, a butterfly inside each wavefront and a fixed-order sum of the four wavefronts through LDS.
//
// The offset of an image in the bank is 64-bit, the image index is clamped, every pixel index is clamped to its image (u8_image.h).  No
// atomics, no scratch, one writer per output element.
#include "u8_image.h"

#define CASCADE_THREADS 256
#define CASCADE_MAX_SUB 8
#define CASCADE_MIN_N 16.0           // fewer counting elements than this: no score (bihome_amd.align.ECC_MIN_N)

struct SubAcc { float r, g, b; unsigned ok; };

// one sub-sample: grid point (X, Y) -> its bilinear value on the three channels (0 under the guard) and its validity
template <bool BYTES>
__device__ __forceinline__ void cascade_sub(SubAcc& a, const U8Image& im, const Hf& Hm, int X, int Y, int Ws, int Hs, float xmax, float ymax) {
    const U8Sample s = u8_sample<BYTES>(im, Hm, X, Y, Ws, Hs, xmax, ymax);
    a.r += s.guard ? 0.0f : s.c[0];
    a.g += s.guard ? 0.0f : s.c[1];
    a.b += s.guard ? 0.0f : s.c[2];
    a.ok += s.valid ? 1u : 0u;
}

// grid (ceil(P * P / CASCADE_THREADS), u8_grid_y(B)); Hs * Ws <= 2^29, 1 <= nx, ny <= CASCADE_MAX_SUB
template <int C, bool BYTES>
__global__ void __launch_bounds__(CASCADE_THREADS) align_prep_warp_kernel(const unsigned char* __restrict__ images, const int* __restrict__ idx, int n_images,
                                                                          int Hs, int Ws, const double* __restrict__ Hg, int B, int P, int nx, int ny,
                                                                          float mean, float std, float* __restrict__ patch, float* __restrict__ cover) {
    const unsigned u = blockIdx.x * CASCADE_THREADS + threadIdx.x;
    if (u >= (unsigned)(P * P)) return;
    const int y = (int)(u / (unsigned)P), x = (int)(u - (unsigned)y * (unsigned)P);
    const unsigned n = (unsigned)Hs * (unsigned)Ws;
    const float xmax = (float)(Ws - 1), ymax = (float)(Hs - 1);
    const int X0 = x * nx, Y0 = y * ny, subs = nx * ny;
    const float inv = 1.0f / ((float)subs * 255.0f);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Hf Hm = load_h(Hg + 9 * (size_t)b);
        const U8Image im = u8_image(images, idx, b, n_images, n);
        SubAcc a = {0.f, 0.f, 0.f, 0u};
        int s = 0, sx = 0, sy = 0;          // sub-sample s sits at column sx, row sy of the cell: row-major
        for (; s + 4 <= subs; s += 4) {
            int X[4], Y[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                X[k] = X0 + sx; Y[k] = Y0 + sy;
                if (++sx == nx) { sx = 0; ++sy; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) cascade_sub<BYTES>(a, im, Hm, X[k], Y[k], Ws, Hs, xmax, ymax);
        }
        for (; s < subs; ++s) {
            cascade_sub<BYTES>(a, im, Hm, X0 + sx, Y0 + sy, Ws, Hs, xmax, ymax);
            if (++sx == nx) { sx = 0; ++sy; }
        }
        u8_store_patch<C>(patch + (size_t)b * C * P * P + u, (size_t)P * P, a.r, a.g, a.b, inv, mean, std);
        if (cover) cover[(size_t)b * P * P + u] = (float)a.ok / (float)subs;          // exactly 1.0f iff every sub-sample is valid
    }
}

#define NCC_SUMS 6          // n, sum w, sum t, sum ww, sum tt, sum wt

// grid (B), CASCADE_THREADS threads: sample b's C * P * P elements, element (c, p) counting iff cover[b, p] == 1.0f
__global__ void __launch_bounds__(CASCADE_THREADS) patch_ncc_kernel(const float* __restrict__ w, const float* __restrict__ t, const float* __restrict__ cover,
                                                                    int C, int PP, double* __restrict__ out) {
    __shared__ double part[CASCADE_THREADS / 64][NCC_SUMS];
    const size_t b = blockIdx.x;
    const float* wb = w + b * C * PP;
    const float* tb = t + b * C * PP;
    const float* cb = cover ? cover + b * PP : nullptr;
    double acc[NCC_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < PP; p += CASCADE_THREADS) {
        if (cb && !(cb[p] == 1.0f)) continue;
        for (int c = 0; c < C; ++c) {
            const double wv = (double)wb[(size_t)c * PP + p], tv = (double)tb[(size_t)c * PP + p];
            acc[0] += 1.0; acc[1] += wv; acc[2] += tv;
            acc[3] += wv * wv; acc[4] += tv * tv; acc[5] += wv * tv;      // (a product of two floats is exact in double)
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NCC_SUMS; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[NCC_SUMS];
#pragma unroll
    for (int k = 0; k < NCC_SUMS; ++k) s[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    const double cnt = s[0];
    const double num = cnt * s[5] - s[1] * s[2], va = cnt * s[3] - s[1] * s[1], vt = cnt * s[4] - s[2] * s[2];
    double* o = out + 8 * b;
#pragma unroll
    for (int k = 0; k < NCC_SUMS; ++k) o[k] = s[k];
    o[6] = (cnt >= CASCADE_MIN_N && va > 0.0 && vt > 0.0) ? num / sqrt(va * vt) : -__builtin_inf();
    o[7] = 0.0;
}

// what both entry points refuse as BH_E_BADARG apart from their NULL pointers and their own extents: a negative batch, a patch without extent
static bool cascade_extents_bad(int count, int p) { return count < 0 || p < 1; }
static bool cascade_patch_unsupported(int c, int p) { return (c != 1 && c != 3) || p % 16 != 0 || p > 256; }

extern "C" {

int bh_align_prep_warp_u8(const uint8_t* images, const int* idx, int n_images, int Hs, int Ws, const double* Hg,
                          int B, int P, int C, int nx, int ny, float mean, float std,
                          float* patch, float* cover, void* stream) {
    if (!images || !Hg || !patch || cascade_extents_bad(B, P) || n_images < 1 || Hs < 1 || Ws < 1 || !(std != 0.0f) || std != std) return BH_E_BADARG;
    // (tap_place's offsets are ints of 4 bytes per pixel, byte offsets inside an image 32-bit)
    if (cascade_patch_unsupported(C, P) || nx < 1 || nx > CASCADE_MAX_SUB || ny < 1 || ny > CASCADE_MAX_SUB || (long long)Hs * Ws > (1ll << 29)) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const dim3 grid((unsigned)(P * P + CASCADE_THREADS - 1) / CASCADE_THREADS, u8_grid_y(B));
    hipStream_t st = bh_stream(stream);
    const bool bytes = (long long)Hs * Ws < 2;                                  // a single-pixel image: no room for 4-byte loads
    u8_flags([&](auto gray, auto by) {
        hipLaunchKernelGGL((align_prep_warp_kernel<gray ? 1 : 3, by>), grid, dim3(CASCADE_THREADS), 0, st, images, idx, n_images, Hs, Ws, Hg, B, P, nx, ny, mean, std, patch, cover);
    }, C == 1, bytes);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_patch_ncc(const float* w, const float* t, const float* cover, int B, int C, int P, double* out, void* stream) {
    if (!w || !t || !out || cascade_extents_bad(B, P)) return BH_E_BADARG;
    if (cascade_patch_unsupported(C, P)) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(patch_ncc_kernel, dim3((unsigned)B), dim3(CASCADE_THREADS), 0, bh_stream(stream), w, t, cover, C, P * P, out);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
