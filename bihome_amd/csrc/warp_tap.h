// The homography warp's per-pixel tap: the ONE spelling of projecting a pixel, the guard, the reciprocal, floor and fraction, the validity of
// the four taps, their weights and offsets.  Every kernel that warps includes it - csrc/warp.hip (every pooling size, the adjoints w.r.t. H
// and w.r.t. the image), the extractor stem's folded warp and warp adjoint (csrc/stem7.hip) and the photometric head (csrc/photo.hip) - so
// forward, adjoint and fused forms agree bitwise on which side of an integer coordinate a pixel falls because they call one function.  The
// bilinear derivative jumps there: with a coordinate left to the compiler's contraction one pixel in ~10^5 took the other branch.  Hence
// `#pragma clang fp contract(off)` around everything but the fused multiply-adds that are written out, in ONE order.
#pragma once
#include "common.h"

struct Hf { float h0, h1, h2, h3, h4, h5, h6, h7, h8; };
__device__ __forceinline__ Hf load_h(const double* __restrict__ Hm) {
    Hf f;
    f.h0 = (float)Hm[0]; f.h1 = (float)Hm[1]; f.h2 = (float)Hm[2]; f.h3 = (float)Hm[3]; f.h4 = (float)Hm[4];
    f.h5 = (float)Hm[5]; f.h6 = (float)Hm[6]; f.h7 = (float)Hm[7]; f.h8 = (float)Hm[8];
    return f;
}

constexpr unsigned TAP_OUTSIDE = 0xFFFFFFFFu;   // offset of a tap outside the image: out of range for the buffer load, which then returns 0

struct Tap4 {
    float u, v, iz, fx, fy;
    float wx0, wx1, wy0, wy1;      // per-axis bilinear weights, 0 where that tap column / row is outside the image
    bool vx0, vx1, vy0, vy1, guard;
    unsigned o00, o01, o10, o11;   // byte offsets of the taps inside one image plane (< 2^32 bytes), TAP_OUTSIDE for a tap outside the image
};

// projection: (u, v) = (qx, qy) / qz of H.(x, y, 1), iz = 1 / qz - or 1 under the guard against qz ~ 0
__device__ __forceinline__ void tap_project(Tap4& t, const Hf& H, int x, int y) {
#pragma clang fp contract(off)      // (u - floor(u) after u = qx * iz is one the compiler would make)
    const float fxp = (float)x, fyp = (float)y;
    const float qx = __builtin_fmaf(H.h0, fxp, __builtin_fmaf(H.h1, fyp, H.h2)), qy = __builtin_fmaf(H.h3, fxp, __builtin_fmaf(H.h4, fyp, H.h5)),
                qz = __builtin_fmaf(H.h6, fxp, __builtin_fmaf(H.h7, fyp, H.h8));
    t.guard = !(fabsf(qz) > 1e-8f);
    float r = __builtin_amdgcn_rcpf(qz);
    r = __builtin_fmaf(__builtin_fmaf(-qz, r, 1.0f), r, r);     // one Newton step: within an ulp of 1/qz, exact for qz = 1
    t.iz = t.guard ? 1.0f : r;
    t.u = qx * t.iz;
    t.v = qy * t.iz;
}

// placement of the four taps around (su, sv) in a w x h plane: fraction, validity, per-axis weights, offsets
__device__ __forceinline__ void tap_place(Tap4& t, float su, float sv, int w, int h) {
#pragma clang fp contract(off)
    const float x0f = floorf(su), y0f = floorf(sv);
    t.fx = su - x0f;
    t.fy = sv - y0f;
    // clamp in float first so that wild coordinates (inf / nan / huge) become plain out-of-bounds integers
    const int x0 = (int)fminf(fmaxf(x0f, -2.0f), (float)w), y0 = (int)fminf(fmaxf(y0f, -2.0f), (float)h);
    t.vx0 = (unsigned)x0 < (unsigned)w; t.vx1 = (unsigned)(x0 + 1) < (unsigned)w;
    t.vy0 = (unsigned)y0 < (unsigned)h; t.vy1 = (unsigned)(y0 + 1) < (unsigned)h;
    t.wx0 = t.vx0 ? 1.0f - t.fx : 0.0f; t.wx1 = t.vx1 ? t.fx : 0.0f;
    t.wy0 = t.vy0 ? 1.0f - t.fy : 0.0f; t.wy1 = t.vy1 ? t.fy : 0.0f;
    const int w4 = 4 * w;
    const int o = y0 * w4 + 4 * x0;
    t.o00 = (t.vx0 && t.vy0) ? (unsigned)o : TAP_OUTSIDE;
    t.o01 = (t.vx1 && t.vy0) ? (unsigned)(o + 4) : TAP_OUTSIDE;
    t.o10 = (t.vx0 && t.vy1) ? (unsigned)(o + w4) : TAP_OUTSIDE;
    t.o11 = (t.vx1 && t.vy1) ? (unsigned)(o + w4 + 4) : TAP_OUTSIDE;
}

// the warp of an image onto its own grid: out(x, y) = bilinear img(H.(x, y, 1))
__device__ __forceinline__ Tap4 make_tap4(const Hf& H, int x, int y, int w, int h) {
    Tap4 t;
    tap_project(t, H, x, y);
    tap_place(t, t.u, t.v, w, h);
    return t;
}

// The photometric head's tap (csrc/photo.hip): the map is written in PATCH coordinates, (x, y) -> origin + Hp.(x, y, 1), and gathers
// from a source plane of its own size wi x hi (the full image, larger than the patch grid).  u / v stay the patch-relative coordinates
// (what the adjoint w.r.t. Hp needs); the taps are placed at origin + (u, v), one add each.
__device__ __forceinline__ Tap4 make_tap4_o(const Hf& H, int x, int y, float ox, float oy, int wi, int hi) {
#pragma clang fp contract(off)
    Tap4 t;
    tap_project(t, H, x, y);
    tap_place(t, ox + t.u, oy + t.v, wi, hi);
    return t;
}

// the weights and the blend of the four taps, spelled out for the same reason: the warp kernels of every pooling size and the stem forward
// that makes its own warped pixels (stem7_fwd_f16_kernel<1, true>) produce bitwise the same image and coverage
__device__ __forceinline__ float tap_wsum(float w00, float w01, float w10, float w11) {      // the warped all-ones mask at this pixel
#pragma clang fp contract(off)
    return ((w00 + w01) + w10) + w11;
}
__device__ __forceinline__ void tap_weights(const Tap4& t, float& w00, float& w01, float& w10, float& w11, float& wsum) {
#pragma clang fp contract(off)
    w00 = t.wx0 * t.wy0; w01 = t.wx1 * t.wy0; w10 = t.wx0 * t.wy1; w11 = t.wx1 * t.wy1;
    wsum = tap_wsum(w00, w01, w10, w11);
}
__device__ __forceinline__ float tap_blend(float p00, float p01, float p10, float p11, float w00, float w01, float w10, float w11) {
#pragma clang fp contract(off)
    float acc = p00 * w00;
    acc = __builtin_fmaf(p01, w01, acc);
    acc = __builtin_fmaf(p10, w10, acc);
    acc = __builtin_fmaf(p11, w11, acc);
    return acc;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const float* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float ldtap(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}
