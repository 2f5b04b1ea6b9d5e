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
#include "common.h"

#define BANK_THREADS 256
#define BANK_MAX_GRID_Y 65535

struct __attribute__((aligned(4))) BankDwords3 { unsigned a, b, c; };

// an index outside [0, n_images) is clamped into it: nothing outside the bank is ever read
__device__ __forceinline__ size_t bank_image(const int* __restrict__ img_idx, int b, int n_images) {
    const int i = img_idx[b];
    return (size_t)(i < 0 ? 0 : (i >= n_images ? n_images - 1 : i));
}

// grid (ceil(n/4 / BANK_THREADS), min(count, BANK_MAX_GRID_Y)), n = Hs*Ws pixels per image, n % 4 == 0
__global__ void __launch_bounds__(BANK_THREADS) bank_gather_vec4_kernel(const unsigned char* __restrict__ bank, const int* __restrict__ img_idx,
                                                                        int count, int n_images, size_t n, float* __restrict__ out) {
    const size_t u = (size_t)blockIdx.x * BANK_THREADS + threadIdx.x;          // unit = pixels 4u .. 4u+3
    if (u >= n / 4) return;
    for (int b = blockIdx.y; b < count; b += gridDim.y) {
        const unsigned char* src = bank + bank_image(img_idx, b, n_images) * n * 3;
        const BankDwords3 d = reinterpret_cast<const BankDwords3*>(src)[u];
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

// grid (ceil(n / BANK_THREADS), min(count, BANK_MAX_GRID_Y)): any n, any alignment
__global__ void __launch_bounds__(BANK_THREADS) bank_gather_scalar_kernel(const unsigned char* __restrict__ bank, const int* __restrict__ img_idx,
                                                                          int count, int n_images, size_t n, float* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * BANK_THREADS + threadIdx.x;
    if (p >= n) return;
    for (int b = blockIdx.y; b < count; b += gridDim.y) {
        const unsigned char* src = bank + (bank_image(img_idx, b, n_images) * n + p) * 3;
        float* dst = out + (size_t)b * 3 * n + p;
        dst[0] = (float)src[0];
        dst[n] = (float)src[1];
        dst[2 * n] = (float)src[2];
    }
}

extern "C" {

int bh_bank_gather_u8(const unsigned char* bank, const int* img_idx, int count, int n_images, int Hs, int Ws, float* out, void* stream) {
    if (!bank || !img_idx || !out || count < 0 || n_images < 1 || Hs < 1 || Ws < 1) return BH_E_BADARG;
    if (count == 0) return BH_OK;
    const size_t n = (size_t)Hs * Ws;
    const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(bank) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const size_t units = vec ? n / 4 : n;
    const size_t gx = (units + BANK_THREADS - 1) / BANK_THREADS;
    if (gx > 0x7fffffffull) return BH_E_UNSUPPORTED;                         // (more than 2^39 pixels in one image)
    const dim3 grid((unsigned)gx, (unsigned)(count < BANK_MAX_GRID_Y ? count : BANK_MAX_GRID_Y));
    hipStream_t st = bh_stream(stream);
    if (vec) hipLaunchKernelGGL(bank_gather_vec4_kernel, grid, dim3(BANK_THREADS), 0, st, bank, img_idx, count, n_images, n, out);
    else hipLaunchKernelGGL(bank_gather_scalar_kernel, grid, dim3(BANK_THREADS), 0, st, bank, img_idx, count, n_images, n, out);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
