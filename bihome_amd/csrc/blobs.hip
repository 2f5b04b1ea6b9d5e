// Occlusion blobs of the pair generator: the reference's CollatorWithBlobs (src/data/transforms.py:746-799) pastes blob-shaped pieces of
// ANOTHER sample's patch_1 into every patch_2.  The blob shape is what porespy's generators.blobs makes of uniform noise (recalled from
// porespy, restated as float64 numpy in bihome_amd/synth.py blob_field): a separable Gaussian blur with scipy's 'reflect' border, a
// standardisation, the normal CDF, a min-max normalisation and a threshold at the porosity.  Noise and source indices are INPUTS: this
// file draws nothing.
//
// Per sample: blur along x, blur along y (4 outputs per thread along the blurred axis: one 16-byte or four 4-byte plane reads feed 16
// FMAs, the tap weights are wave-uniform kernel arguments), mean / variance / minimum / maximum as in-workgroup reductions with the sums
// in double, then erfc at the minimum, the maximum and per pixel, the mask, and the select into patch_2.  P <= 128: one workgroup per
// sample, both planes in LDS (2 x 64 KiB at P = 128).  P = 256: the same three steps as three launches through two global scratch planes.
// No atomics and a fixed summation order everywhere: two calls on the same inputs are bitwise equal.
#include "common.h"

#define BLOB_MAX_P 256
#define BLOB_LDS_P 128                 // largest P whose two planes fit one workgroup's LDS
#define BLOB_K0 (BLOB_MAX_P + 8)        // index of tap 0: a group of four source values looks up to six taps past the radius r <= P
#define BLOB_TAPS (2 * BLOB_K0 + 4)

// w[BLOB_K0 + k] = exp(-0.5 (k / sigma)^2) / sum for |k| <= r (made on the host in double, rounded once), 0 beyond: indexed by the
// SIGNED tap, so that the seven weights a group needs are seven consecutive words (scalar loads that merge)
struct BlobTaps { float w[BLOB_TAPS]; };
static void blob_make_taps(double sigma, int r, BlobTaps& taps) {
    double e[BLOB_MAX_P + 1], sum = 0.0;
    for (int k = 0; k <= r; ++k) {
        e[k] = exp(-0.5 * ((double)k / sigma) * ((double)k / sigma));
        sum += k ? 2.0 * e[k] : e[k];
    }
    for (int i = 0; i < BLOB_TAPS; ++i) {
        const int k = i < BLOB_K0 ? BLOB_K0 - i : i - BLOB_K0;
        taps.w[i] = k <= r ? (float)(e[k] / sum) : 0.f;
    }
}

// The four source values at positions s..s+3 (s % 4 == 0) of a line of P values under scipy's 'reflect' border (d c b a | a b c d |
// d c b a): P % 4 == 0, so a group lies wholly inside or wholly outside, and a group outside is the reversed group at the mirrored
// place.  -P <= s <= 2P - 4 (r <= P: one reflection serves).  ROWS: the line is a row (16-byte read), else a column of row stride P.
template <bool ROWS>
__host__ __device__ __forceinline__ float4 blob_group(const float* __restrict__ line, int s, int P) {
    const bool out = s < 0 || s >= P;
    const int g = s < 0 ? -s - 4 : (s >= P ? 2 * P - 4 - s : s);
    float4 a;
    if constexpr (ROWS) a = *reinterpret_cast<const float4*>(line + g);
    else a = make_float4(line[(size_t)g * P], line[(size_t)(g + 1) * P], line[(size_t)(g + 2) * P], line[(size_t)(g + 3) * P]);
    return out ? make_float4(a.w, a.z, a.y, a.x) : a;
}

// One unit of a blur pass: four consecutive outputs o0..o0+3 (o0 % 4 == 0) of one line.  out[j] = sum_k w[|k|] in[o0 + j + k]; source
// group m holds positions o0 + 4m + i, so its weight for output j is w[|4m + i - j|] - uniform over the wave, and every output adds
// its taps in the same order k = -r..r (a zero weight adds nothing): a constant plane stays exactly constant.  `bias` is subtracted
// from every source value (0.5 on the first pass: the blur of noise - 0.5 is g - 0.5, and sums of centred values round 100x finer
// against the field's spread than sums of values near 0.5; the standardisation that follows removes any constant).
template <bool ROWS>
__host__ __device__ __forceinline__ float4 blob_blur4(const float* __restrict__ line, int o0, int P, int r, const BlobTaps& taps, float bias) {
    const int M = (r + 3) >> 2;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int m = -M; m <= M; ++m) {
        const float4 a4 = blob_group<ROWS>(line, o0 + 4 * m, P);
        const float a[4] = {a4.x - bias, a4.y - bias, a4.z - bias, a4.w - bias};
        const float* wk = taps.w + (BLOB_K0 - 3 + 4 * m);          // wk[t] = w[|4m - 3 + t|], t = 0..6
        const float c[7] = {wk[0], wk[1], wk[2], wk[3], wk[4], wk[5], wk[6]};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(c[i - j + 3], a[i], acc[j]);
    }
    return make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// units [u0, u1) of the pass along x: unit u = (row u / (P/4), columns 4 (u % (P/4)) ...).  src, dst: planes [P][P].
__host__ __device__ __forceinline__ void blob_pass_x(const float* __restrict__ src, float* __restrict__ dst, int P, int r, const BlobTaps& taps,
                                            int u0, int u1, int step) {
    const int q = P >> 2;
    for (int u = u0; u < u1; u += step) {
        const int y = u / q, x0 = (u - y * q) * 4;
        *reinterpret_cast<float4*>(dst + (size_t)y * P + x0) = blob_blur4<true>(src + (size_t)y * P, x0, P, r, taps, 0.5f);
    }
}
// units of the pass along y: unit u = (column u % P, rows 4 (u / P) ...): consecutive lanes read consecutive columns
__host__ __device__ __forceinline__ void blob_pass_y(const float* __restrict__ src, float* __restrict__ dst, int P, int r, const BlobTaps& taps,
                                            int u0, int u1, int step) {
    for (int u = u0; u < u1; u += step) {
        const int yq = u / P, x = u - yq * P, y0 = yq * 4;
        const float4 o = blob_blur4<false>(src + x, y0, P, r, taps, 0.f);
        float* q = dst + (size_t)y0 * P + x;
        q[0] = o.x; q[P] = o.y; q[2 * (size_t)P] = o.z; q[3 * (size_t)P] = o.w;
    }
}

// every thread gets the workgroup's total (fixed order: lanes by butterfly, then the waves in turn); red: >= 16 doubles of LDS
__device__ __forceinline__ double blob_block_sum(double v, double* red) {
    v = wave_sum(v);
    const int nw = (blockDim.x + 63) >> 6;
    __syncthreads();                                   // (red may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[w];
    return t;
}
__device__ __forceinline__ float blob_block_max(float v, double* red) {
    v = wave_max(v);
    const int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)v;
    __syncthreads();
    float t = (float)red[0];
    for (int w = 1; w < nw; ++w) t = fmaxf(t, (float)red[w]);
    return t;
}

__device__ __forceinline__ double blob_cdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// The whole workgroup, sample b: g = the blurred plane (LDS or global) -> field (NULL ok), mask, and the select into patch_2.
// A flat plane (std == 0, or equal CDF values at the minimum and the maximum) has no blobs: field 1, mask 0, patch_2 untouched.
__device__ __forceinline__ void blob_finish(const float* __restrict__ g, int b, int B, int P, int C, double porosity,
                                            const int* __restrict__ other, const float* __restrict__ patch1, float* __restrict__ patch2,
                                            float* __restrict__ mask, float* __restrict__ field, double* red) {
    const int n = P * P, t = threadIdx.x, nt = blockDim.x;
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = t; i < n; i += nt) {
        const float v = g[i];
        s += (double)v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    const double mean = blob_block_sum(s, red) / n;
    hi = blob_block_max(hi, red);
    lo = -blob_block_max(-lo, red);
    double q = 0.0;
    for (int i = t; i < n; i += nt) {
        const double d = (double)g[i] - mean;
        q += d * d;
    }
    const double sd = sqrt(blob_block_sum(q, red) / n);                 // population std
    double umin = 0.0, scale = 0.0;
    // (constant noise comes out of both passes exactly constant: every output adds the same products in the same order, tap by tap)
    bool flat = !(hi > lo) || !(sd > 0.0);
    if (!flat) {
        umin = blob_cdf(((double)lo - mean) / sd);
        const double umax = blob_cdf(((double)hi - mean) / sd);
        flat = !(umax > umin);
        if (!flat) scale = umax - umin;
    }
    int src = other[b];
    if ((unsigned)src >= (unsigned)B) src = b;                          // an index outside the batch is never followed
    const size_t pp = (size_t)n;
    for (int i = t; i < n; i += nt) {
        double u = 1.0;
        if (!flat) {
            u = (blob_cdf(((double)g[i] - mean) / sd) - umin) / scale;       // (a quotient: exactly 1 at the maximum)
            u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
        }
        const bool in = u < porosity;
        if (field) field[(size_t)b * pp + i] = (float)u;
        mask[(size_t)b * pp + i] = in ? 1.f : 0.f;
        if (in)
            for (int c = 0; c < C; ++c) patch2[((size_t)b * C + c) * pp + i] = patch1[((size_t)src * C + c) * pp + i];
    }
}

// P <= BLOB_LDS_P: grid B, block min(1024, P*P/4), dynamic LDS 2 P P floats
__global__ void __launch_bounds__(1024) blobs_fused_kernel(const float* __restrict__ noise, const int* __restrict__ other,
                                                           const float* __restrict__ patch1, float* __restrict__ patch2,
                                                           float* __restrict__ mask, float* __restrict__ field, int B, int P, int C,
                                                           int r, double porosity, const BlobTaps taps) {
    extern __shared__ __align__(16) float planes[];
    __shared__ double red[16];
    const int b = blockIdx.x, n = P * P, t = threadIdx.x, nt = blockDim.x;
    float* X = planes;
    float* Y = planes + n;
    const float4* src = reinterpret_cast<const float4*>(noise + (size_t)b * n);
    for (int i = t; i < n / 4; i += nt) reinterpret_cast<float4*>(X)[i] = src[i];
    __syncthreads();
    blob_pass_x(X, Y, P, r, taps, t, n / 4, nt);
    __syncthreads();
    blob_pass_y(Y, X, P, r, taps, t, n / 4, nt);
    __syncthreads();
    blob_finish(X, b, B, P, C, porosity, other, patch1, patch2, mask, field, red);
}

// P > BLOB_LDS_P: grid (ceil(P*P/4 / 256), B), block 256, one unit per thread; then blobs_finish_kernel, grid B, block 1024
template <bool ROWS>
__global__ void __launch_bounds__(256) blobs_pass_kernel(const float* __restrict__ src, float* __restrict__ dst, int P, int r,
                                                         const BlobTaps taps) {
    const size_t off = (size_t)blockIdx.y * P * P;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= P * P / 4) return;
    if constexpr (ROWS) blob_pass_x(src + off, dst + off, P, r, taps, u, u + 1, 1);
    else blob_pass_y(src + off, dst + off, P, r, taps, u, u + 1, 1);
}
__global__ void __launch_bounds__(1024) blobs_finish_kernel(const float* __restrict__ g, const int* __restrict__ other,
                                                            const float* __restrict__ patch1, float* __restrict__ patch2,
                                                            float* __restrict__ mask, float* __restrict__ field, int B, int P, int C,
                                                            double porosity) {
    __shared__ double red[16];
    blob_finish(g + (size_t)blockIdx.x * P * P, blockIdx.x, B, P, C, porosity, other, patch1, patch2, mask, field, red);
}

extern "C" {

size_t bh_synth_blobs_scratch_floats(int B, int P) {
    if (B < 1 || P <= BLOB_LDS_P || P > BLOB_MAX_P) return 0;
    return (size_t)2 * B * P * P;
}

int bh_synth_blobs(const float* noise, const int* other, const float* patch1, float* patch2, float* mask, float* field,
                   float* scratch, int B, int C, int P, double sigma, double porosity, void* stream) {
    if (!noise || !other || !patch1 || !patch2 || !mask || B < 2 || (C != 1 && C != 3) || !(sigma > 0.0) || !(sigma < 1e30) ||
        !(porosity >= 0.0 && porosity <= 1.0))
        return BH_E_BADARG;
    if (P < 16 || P % 16 || P > BLOB_MAX_P) return BH_E_UNSUPPORTED;
    const double r4 = 4.0 * sigma + 0.5;
    if (r4 > (double)P + 1.0) return BH_E_UNSUPPORTED;                   // radius > P (blobiness < 0.1): more than one reflection
    const int r = (int)r4;
    if (r > P) return BH_E_UNSUPPORTED;
    if (P > BLOB_LDS_P && !scratch) return BH_E_BADARG;
    BlobTaps taps;
    blob_make_taps(sigma, r, taps);
    hipStream_t st = bh_stream(stream);
    if (P <= BLOB_LDS_P) {
        const size_t lds = (size_t)2 * P * P * sizeof(float);
        static unsigned long long attr_devs = 0;
        if (bh_device_once(attr_devs)) {
            hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(blobs_fused_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 2 * BLOB_LDS_P * BLOB_LDS_P * (int)sizeof(float));
            if (e1 != hipSuccess) return (int)e1;
        }
        const int threads = P * P / 4 < 1024 ? P * P / 4 : 1024;
        hipLaunchKernelGGL(blobs_fused_kernel, dim3(B), dim3(threads), lds, st, noise, other, patch1, patch2, mask, field, B, P, C, r,
                           porosity, taps);
        BH_LAUNCH_CHECK();
        return BH_OK;
    }
    float* s0 = scratch;
    float* s1 = scratch + (size_t)B * P * P;
    const dim3 grid((P * P / 4 + 255) / 256, B);
    hipLaunchKernelGGL(blobs_pass_kernel<true>, grid, dim3(256), 0, st, noise, s0, P, r, taps);
    BH_LAUNCH_CHECK();
    hipLaunchKernelGGL(blobs_pass_kernel<false>, grid, dim3(256), 0, st, (const float*)s0, s1, P, r, taps);
    BH_LAUNCH_CHECK();
    hipLaunchKernelGGL(blobs_finish_kernel, dim3(B), dim3(1024), 0, st, (const float*)s1, other, patch1, patch2, mask, field, B, P, C,
                       porosity);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
