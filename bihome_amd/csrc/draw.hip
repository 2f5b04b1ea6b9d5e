// Counter-based draws of the pair generator: sample n of seed s gets every random quantity as a pure function of (s, n), so a run can
// name its samples - resume onto its stream, or split one global batch over any number of ranks.  The function is Philox4x64-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the generator numpy has as np.random.Philox: word k of sample n
// for purpose p is element k % 4 of philox4x64_10(counter = (k / 4 + 1, n, 0, 0), key = (seed, p)) - include/bihome.h states the stream
// and bihome_amd/synth.py counter_draws is its numpy restatement, which every output here equals bit for bit.
//
// Two kernels: the parameters (one thread per sample: 3 Philox blocks, 9 with photometric records) and the blob noise (one thread per
// Philox block = four consecutive pixels = one 16-byte store).  No atomics, no scratch, no allocation, no synchronisation.
#include "common.h"

typedef unsigned long long u64;

#define PHILOX_M0 0xD2E7470EE14C6C93ull
#define PHILOX_M1 0xCA5A826395121157ull
#define PHILOX_W0 0x9E3779B97F4A7C15ull
#define PHILOX_W1 0xBB67AE8584CAA73Bull

#define DRAW_PARAM_WORDS 12            // purpose 0: words 0..11 are index, centre, blob source and the eight corner offsets
#define DRAW_PHOTO_WORDS 36            // ... 12..22 and 24..34 the uniforms of the two photometric records (23 and 35 unused)

// (the host forms serve a CPU build of the per-sample bodies below: the same bits without a GPU)
__host__ __device__ __forceinline__ u64 mulhi64(u64 a, u64 b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

// ten rounds; the key is bumped between rounds (nine times)
__host__ __device__ __forceinline__ void philox4x64_10(u64 c0, u64 c1, u64 c2, u64 c3, u64 k0, u64 k1, u64* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 hi0 = mulhi64(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const u64 hi1 = mulhi64(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// integer in [0, r): the high half of word * r (r < 2^31)
__host__ __device__ __forceinline__ int draw_int(u64 word, int r) { return (int)mulhi64(word, (u64)r); }
// numpy's Generator.random(): 53 bits
__host__ __device__ __forceinline__ double draw_double(u64 word) { return (double)(word >> 11) * 0x1p-53; }

// One PhotometricDistortSimple record from 11 uniforms: synth_gpu.photometric_records' formulas in double, each product and sum rounded
// on its own (a fused lo + (hi - lo) u differs from numpy in the last bit), the result rounded once to float.
__host__ __device__ __forceinline__ void draw_photo_record(const u64* __restrict__ w, double md, float* __restrict__ rec) {
#pragma clang fp contract(off)
    double u[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) u[i] = draw_double(w[i]);
    const double lower = 1.0 - md / 32 * 0.5, upper = 1.0 + md / 32 * 0.5;
    const double br = u[0] >= 0.5 ? -md + (2 * md) * u[1] : 0.0;
    const bool first = u[2] >= 0.5;
    const double con = u[3] >= 0.5 ? lower + (upper - lower) * u[4] : 1.0;
    const double sat = u[5] >= 0.5 ? lower + (upper - lower) * u[6] : 1.0;
    const double hue = u[7] >= 0.5 ? -md / 2 + md * u[8] : 0.0;
    double perm = 0.0;
    if (md > 0 && u[9] >= 0.5) {
        perm = floor(6 * u[10]);
        perm = perm > 5.0 ? 5.0 : perm;
    }
    rec[0] = (float)br;
    rec[1] = (float)(first ? con : 1.0);
    rec[2] = (float)sat;
    rec[3] = (float)hue;
    rec[4] = (float)(first ? 1.0 : con);
    rec[5] = (float)perm;
}

// Sample b of the call: everything the parameter kernel writes for it.  xr / yr: the number of patch positions along x / y (>= 1).
__host__ __device__ __forceinline__ void draw_sample(int b, u64 seed, u64 first, int B, int n_images, int xr, int yr, int rho, float max_delta,
                                                     int* __restrict__ img_idx, float* __restrict__ origin, float* __restrict__ delta,
                                                     float* __restrict__ photo, int* __restrict__ other) {
    const u64 n = first + (u64)b;
    u64 w[DRAW_PHOTO_WORDS];
#pragma unroll
    for (int k = 0; k < DRAW_PARAM_WORDS / 4; ++k) philox4x64_10((u64)k + 1, n, 0, 0, seed, 0, w + 4 * k);
    img_idx[b] = draw_int(w[0], n_images);
    // the patch centre is rho + P/2 + draw, the origin P/2 less (transforms.py:505-506)
    origin[2 * (size_t)b] = (float)(rho + draw_int(w[1], xr));
    origin[2 * (size_t)b + 1] = (float)(rho + draw_int(w[2], yr));
    if (other) {
        const int r = draw_int(w[3], B - 1);
        other[b] = r + (r >= b ? 1 : 0);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) delta[(size_t)b * 8 + i] = (float)(draw_int(w[4 + i], 2 * rho) - rho);      // transforms.py:538
    if (photo) {
#pragma unroll
        for (int k = DRAW_PARAM_WORDS / 4; k < DRAW_PHOTO_WORDS / 4; ++k) philox4x64_10((u64)k + 1, n, 0, 0, seed, 0, w + 4 * k);
        draw_photo_record(w + 12, (double)max_delta, photo + (size_t)b * 12);
        draw_photo_record(w + 24, (double)max_delta, photo + (size_t)b * 12 + 6);
    }
}

// Philox block j of sample b's noise plane of pp = P * P floats: pixels 4j .. 4j + 3 (4j < pp).  VEC: pp % 4 == 0 and a 16-byte aligned
// base, so every block is one whole float4 store.
template <bool VEC>
__host__ __device__ __forceinline__ void draw_noise_block(size_t j, int b, u64 seed, u64 first, size_t pp, float* __restrict__ noise) {
    u64 w[4];
    philox4x64_10((u64)j + 1, first + (u64)b, 0, 0, seed, 1, w);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)(w[i] >> 40) * 0x1p-24f;                  // 24 bits: exact
    float* q = noise + (size_t)b * pp + 4 * j;
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * j + i < pp) q[i] = v[i];
    }
}

// grid ceil(B / 64), block 64: thread = sample
__global__ void __launch_bounds__(64) draw_params_kernel(u64 seed, u64 first, int B, int n_images, int xr, int yr, int rho, float max_delta,
                                                         int* __restrict__ img_idx, float* __restrict__ origin, float* __restrict__ delta,
                                                         float* __restrict__ photo, int* __restrict__ other) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) draw_sample(b, seed, first, B, n_images, xr, yr, rho, max_delta, img_idx, origin, delta, photo, other);
}

// grid (ceil(blocks per sample / 256), min(B, 65535)), block 256: thread = Philox block j of the samples blockIdx.y, + gridDim.y, ...
template <bool VEC>
__global__ void __launch_bounds__(256) draw_noise_kernel(u64 seed, u64 first, int B, size_t pp, float* __restrict__ noise) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (4 * j >= pp) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) draw_noise_block<VEC>(j, b, seed, first, pp, noise);
}

extern "C" {

// seed, first: unsigned 64-bit words (size_t: the header's one unsigned 64-bit scalar type)
static_assert(sizeof(size_t) == 8, "bh_synth_draw passes its 64-bit words as size_t");

int bh_synth_draw(size_t seed_word, size_t first_word, int B, int n_images, int Hs, int Ws, int P, int rho, float max_delta,
                  int* img_idx, float* origin, float* delta, float* photo, float* noise, int* other, void* stream) {
    const u64 seed = (u64)seed_word, first = (u64)first_word;
    // (the negative count and the empty batch of this entry point are exercised by tests/test_counter_draws_cpu.py / _gpu.py)
    if (!(B >= 0) || n_images < 1 || rho < 1 || P < 1) return BH_E_BADARG;
    const long long need = (long long)P + 2ll * rho;
    if ((long long)Hs < need || (long long)Ws < need) return BH_E_BADARG;            // (so 2 rho and P fit an int)
    if ((noise != nullptr) != (other != nullptr)) return BH_E_BADARG;
    if (B == 0) return BH_OK;
    if (!img_idx || !origin || !delta) return BH_E_BADARG;
    if (noise && B < 2) return BH_E_BADARG;
    hipStream_t st = bh_stream(stream);
    const int half = P / 2;
    const int xr = Ws - 2 * rho - 2 * half + 1, yr = Hs - 2 * rho - 2 * half + 1;
    hipLaunchKernelGGL(draw_params_kernel, dim3((B + 63) / 64), dim3(64), 0, st, seed, first, B, n_images, xr, yr, rho, max_delta, img_idx,
                       origin, delta, photo, other);
    BH_LAUNCH_CHECK();
    if (noise) {
        const size_t pp = (size_t)P * P;
        const size_t blocks = (pp + 3) / 4;
        const dim3 grid((unsigned)((blocks + 255) / 256), (unsigned)(B < 65535 ? B : 65535));
        if (pp % 4 == 0 && (reinterpret_cast<uintptr_t>(noise) & 15) == 0)
            hipLaunchKernelGGL(draw_noise_kernel<true>, grid, dim3(256), 0, st, seed, first, B, pp, noise);
        else
            hipLaunchKernelGGL(draw_noise_kernel<false>, grid, dim3(256), 0, st, seed, first, B, pp, noise);
        BH_LAUNCH_CHECK();
    }
    return BH_OK;
}

}  // extern "C"
