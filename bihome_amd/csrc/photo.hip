// Photometric head (src/heads/PhotometricHead.py, Nguyen et al.'s unsupervised baseline): patch_hat = crop of warp_image(image_1, H_hat) at
// the patch corners, and its adjoint w.r.t. the homography.  Only the crop window is computed: with Hp = four_point_to_homography of the
// patch corners [[0,0],[P,0],[P,P],[0,P]] and o the integer top-left corner of the patch in the image, H_hat.(o + u) = o + Hp.u for every
// patch pixel u, so out[b,c,j,i] = bilinear img[b,c](o_b + Hp_b.(i, j, 1)), zero padding outside the Hi x Wi image (kornia.warp_perspective,
// align_corners=True).  P x P samples per plane instead of the Hi x Wi the reference warps before cropping.
// Tile = 16 x 16 output pixels per 256-thread block; a row of 16 pixels is one coalesced 64-byte store.  Gathers are buffer loads on a
// per-plane resource: a tap outside the image carries an out-of-range offset and reads 0 without a branch.
#include "common.h"
#include "warp_tap.h"

// grid (P/16, P/16, B), block 256 = 16 x 16
__global__ void __launch_bounds__(256) photo_warp_fwd_kernel(const float* __restrict__ img, const double* __restrict__ Hp64,
                                                             const float* __restrict__ origin, int C, int Hi, int Wi, int P,
                                                             float* __restrict__ out) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    const Hf H = load_h(Hp64 + (size_t)b * 9);
    const Tap4 t = make_tap4_o(H, x, y, origin[2 * b], origin[2 * b + 1], Wi, Hi);
    float w00, w01, w10, w11, ws_;
    tap_weights(t, w00, w01, w10, w11, ws_);
    const unsigned plane = (unsigned)Hi * (unsigned)Wi;
    for (int c = 0; c < C; ++c) {
        const __amdgpu_buffer_rsrc_t rs = plane_rsrc(img + ((size_t)b * C + c) * plane, plane * 4u);
        const float p00 = ldtap(rs, t.o00), p01 = ldtap(rs, t.o01), p10 = ldtap(rs, t.o10), p11 = ldtap(rs, t.o11);
        out[(((size_t)b * C + c) * P + y) * P + x] = tap_blend(p00, p01, p10, p11, w00, w01, w10, w11);
    }
}

// adjoint w.r.t. Hp: per pixel dL/du, dL/dv (summed over channels) -> 9 double sums per sample (warp_bwd_kernel's arithmetic).
// grid (P/16, P/16, B); deterministic mode: grid (1, 1, B) - one workgroup walks every tile of its sample and is the only writer of gH[b]
__global__ void __launch_bounds__(256) photo_warp_bwd_kernel(const float* __restrict__ img, const double* __restrict__ Hp64,
                                                             const float* __restrict__ origin, const float* __restrict__ g_out, int C,
                                                             int Hi, int Wi, int P, double* __restrict__ gH) {
    __shared__ double part[4][9];
    const int b = blockIdx.z;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const Hf H = load_h(Hp64 + (size_t)b * 9);
    const float ox = origin[2 * b], oy = origin[2 * b + 1];
    const unsigned plane = (unsigned)Hi * (unsigned)Wi;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int by = blockIdx.y; by < P / 16; by += gridDim.y)
    for (int bx = blockIdx.x; bx < P / 16; bx += gridDim.x) {
        const int x = bx * 16 + tx, y = by * 16 + ty;
        const Tap4 t = make_tap4_o(H, x, y, ox, oy, Wi, Hi);
        float gu = 0.0f, gv = 0.0f;
        for (int c = 0; c < C; ++c) {
            const __amdgpu_buffer_rsrc_t rs = plane_rsrc(img + ((size_t)b * C + c) * plane, plane * 4u);
            const float go = g_out[(((size_t)b * C + c) * P + y) * P + x];
            // taps outside the image load 0 and the per-axis weights of rows / columns outside are 0: they contribute nothing
            // (grid_sampler_2d_backward)
            const float p00 = ldtap(rs, t.o00), p01 = ldtap(rs, t.o01), p10 = ldtap(rs, t.o10), p11 = ldtap(rs, t.o11);
            gu += go * ((p01 - p00) * t.wy0 + (p11 - p10) * t.wy1);
            gv += go * ((p10 - p00) * t.wx0 + (p11 - p01) * t.wx1);
        }
        // u = qx*iz, v = qy*iz (patch-relative: the origin is a constant offset), iz = 1/qz (or 1 under the guard)
        const double fx = (double)x, fy = (double)y, dgu = (double)gu, dgv = (double)gv, diz = (double)t.iz;
        const double a = dgu * diz, bq = dgv * diz;
        const double gz = t.guard ? 0.0 : -(dgu * (double)t.u + dgv * (double)t.v) * diz;
        acc[0] += a * fx; acc[1] += a * fy; acc[2] += a;
        acc[3] += bq * fx; acc[4] += bq * fy; acc[5] += bq;
        acc[6] += gz * fx; acc[7] += gz * fy; acc[8] += gz;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int k = 0; k < 9; ++k) part[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 9)
        atomicAdd(gH + (size_t)b * 9 + threadIdx.x, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

extern "C" {

int bh_photo_warp_fwd(const float* img, const double* Hp64, const float* origin, int B, int C, int Hi, int Wi, int P, float* out,
                      int flags, void* stream) {
    (void)flags;                  // (a gather: one writer per output pixel in either mode)
    if (!img || !Hp64 || !origin || !out || B < 0 || C < 1 || Hi < 1 || Wi < 1 || P < 1) return BH_E_BADARG;
    if ((P % 16) || (size_t)Hi * (size_t)Wi * 4u >= 0xFFFFFFFFull) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(photo_warp_fwd_kernel, dim3(P / 16, P / 16, B), dim3(256), 0, bh_stream(stream), img, Hp64, origin, C, Hi, Wi, P,
                       out);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_photo_warp_bwd(const float* img, const double* Hp64, const float* origin, const float* g_out, int B, int C, int Hi, int Wi,
                      int P, double* gH, int flags, void* stream) {
    if (!img || !Hp64 || !origin || !g_out || !gH || B < 0 || C < 1 || Hi < 1 || Wi < 1 || P < 1) return BH_E_BADARG;
    if ((P % 16) || (size_t)Hi * (size_t)Wi * 4u >= 0xFFFFFFFFull) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    const dim3 grid = (flags & BH_F_DETERMINISTIC) ? dim3(1, 1, B) : dim3(P / 16, P / 16, B);
    hipLaunchKernelGGL(photo_warp_bwd_kernel, grid, dim3(256), 0, bh_stream(stream), img, Hp64, origin, g_out, C, Hi, Wi, P, gH);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
