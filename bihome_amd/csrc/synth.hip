// GPU-side synthetic pair generator: the reference's CPU data pipeline for one sample (src/data/transforms.py:
// HomographyNetPrep :441-725 -> crop patch_1, warp the image with the 4-point homography and crop patch_2;
// DictToGrayscale :344-354; DictStandardize :369-378; PhotometricDistortSimple :296-330 - brightness, contrast, HSV
// saturation / hue, channel permutation) as ONE kernel over resident base images.  At >= 2k pairs/s per GPU the 8 cv2 DataLoader workers of the
// reference cannot keep up; this reuses the homography-warp arithmetic of csrc/warp.hip.
// HBM-bound: reads <= 4 taps x 3 channels of the base image per output pixel (cache-resident), writes 8 B/pixel per patch channel
// (C = 1: grayscale patches; C = 3: the RGB patches of BASELINE.json configs[4]) and 8 B/pixel more for the 'all_points' target
// (HomographyNetPrep, transforms.py:635-685), which costs no extra read: it is the warp's own coordinate minus the pixel's.
#include "common.h"

// One PhotometricDistortSimple record (bihome_amd/synth.py draw_photometric; transforms.py:296-330) applied to an RGB
// triple: brightness, contrast (before the HSV part), saturation / hue in OpenCV's float HSV (cvtColor CV_32F: V = max,
// S = (V - min) / (|V| + eps), H in degrees), contrast (after), channel permutation.  photo_rgb leaves the permuted triple in
// (o0, o1, o2); photo_gray is its grayscale value 0.299 R' + 0.587 G' + 0.114 B' (transforms.py:351-353).
struct PhotoRec { float br, c1, sat, hue, c2; int perm; };

__device__ __forceinline__ void photo_rgb(float r, float g, float b, const PhotoRec& p, float& o0, float& o1, float& o2) {
    constexpr float EPS = 1.1920929e-07f;
    r = (r + p.br) * p.c1; g = (g + p.br) * p.c1; b = (b + p.br) * p.c1;
    // RGB -> HSV
    const float v = fmaxf(fmaxf(r, g), b), vmin = fminf(fminf(r, g), b);
    const float diff = v - vmin;
    float s = diff / (fabsf(v) + EPS);
    const float d = 60.0f / (diff + EPS);
    float h = (v == r) ? (g - b) * d : ((v == g) ? (b - r) * d + 120.0f : (r - g) * d + 240.0f);
    if (h < 0.0f) h += 360.0f;
    s *= p.sat;
    if (p.hue != 0.0f) {
        h += p.hue;
        if (h > 360.0f) h -= 360.0f;
        if (h < 0.0f) h += 360.0f;
    }
    // HSV -> RGB (sector table)
    float R = v, G = v, B = v;
    if (s != 0.0f) {
        float hh = h * (6.0f / 360.0f);
        if (hh < 0.0f || hh >= 6.0f) hh -= floorf(hh / 6.0f) * 6.0f;
        int sector = (int)floorf(hh);
        float fr = hh - (float)sector;
        if ((unsigned)sector >= 6u) { sector = 0; fr = 0.0f; }
        const float t1 = v * (1.0f - s), t2 = v * (1.0f - s * fr), t3 = v * (1.0f - s * (1.0f - fr));
        switch (sector) {
            case 0: R = v;  G = t3; B = t1; break;
            case 1: R = t2; G = v;  B = t1; break;
            case 2: R = t1; G = v;  B = t3; break;
            case 3: R = t1; G = t2; B = v;  break;
            case 4: R = t3; G = t1; B = v;  break;
            default: R = v; G = t1; B = t2; break;
        }
    }
    R *= p.c2; G *= p.c2; B *= p.c2;
    // out[c] = in[perm[c]] for perm in ((0,1,2),(0,2,1),(1,0,2),(1,2,0),(2,0,1),(2,1,0))
    o0 = R; o1 = G; o2 = B;
    switch (p.perm) {
        case 1: o1 = B; o2 = G; break;
        case 2: o0 = G; o1 = R; break;
        case 3: o0 = G; o1 = B; o2 = R; break;
        case 4: o0 = B; o1 = R; o2 = G; break;
        case 5: o0 = B; o2 = R; break;
        default: break;
    }
}

__device__ __forceinline__ float photo_gray(float r, float g, float b, const PhotoRec& p) {
    float o0, o1, o2;
    photo_rgb(r, g, b, p, o0, o1, o2);
    return o0 * 0.299f + o1 * 0.587f + o2 * 0.114f;
}

// DictStandardize (transforms.py:377) as a product, a difference and a product, never contracted: the rounding every plane of the
// generator has always had, and what keeps patch_1 bitwise the crop of bh_synth_image's plane whatever surrounds the expression
__device__ __forceinline__ float standardise(float g, float mean, float inv_std) {
#pragma clang fp contract(off)
    return (g * (1.0f / 255.0f) - mean) * inv_std;
}

// grid (P/16, P/16, B), block 256 = 16x16.  photo: [B][2 images][6] records or NULL (no distortion).  One body for every form of the
// generator: C = 1 writes grayscale patches [B,1,P,P], C = 3 the permuted, distorted channels themselves [B,3,P,P]; TGT also writes the
// perspective field target[B,2,P,P].  C and TGT are compile-time so that the C = 1, no-target instance does exactly the
// floating-point work bh_synth_pairs has always done.  Every store is a 16-lane row of consecutive floats, plane by plane.
template <int C, bool TGT>
__global__ void __launch_bounds__(256) synth_batch_kernel(const float* __restrict__ images, const int* __restrict__ img_idx,
                                                          const float* __restrict__ origin, const double* __restrict__ Hp,
                                                          const float* __restrict__ photo, int Hs, int Ws, int P, float mean,
                                                          float inv_std, float* __restrict__ p1, float* __restrict__ p2,
                                                          float* __restrict__ target) {
    static_assert(C == 1 || C == 3, "grayscale or RGB patches");
    const int b = blockIdx.z;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    const float* img = images + (size_t)img_idx[b] * 3 * Hs * Ws;
    const size_t plane = (size_t)Hs * Ws, pp = (size_t)P * P;
    const int x0 = (int)origin[b * 2], y0 = (int)origin[b * 2 + 1];
    PhotoRec r1 = {0.f, 1.f, 1.f, 0.f, 1.f, 0}, r2 = r1;
    if (photo) {
        const float* q = photo + (size_t)b * 12;
        r1 = {q[0], q[1], q[2], q[3], q[4], (int)q[5]};
        r2 = {q[6], q[7], q[8], q[9], q[10], (int)q[11]};
    }
    struct Px { float c[C]; };
    // the distortion is applied to the IMAGE before it is warped (transforms.py:474-481 precede :571): per tap
    auto tap = [&](int yy, int xx, const PhotoRec& r) -> Px {
        const float* q = img + (size_t)yy * Ws + xx;
        if constexpr (C == 1) {
            if (!photo) return {{q[0] * 0.299f + q[plane] * 0.587f + q[2 * plane] * 0.114f}};      // transforms.py:351-353
            return {{photo_gray(q[0], q[plane], q[2 * plane], r)}};
        } else {
            Px o = {{q[0], q[plane], q[2 * plane]}};
            if (photo) photo_rgb(q[0], q[plane], q[2 * plane], r, o.c[0], o.c[1], o.c[2]);
            return o;
        }
    };
    const size_t pix = (size_t)y * P + x;
    // patch_1: plain crop at `origin`
    {
        const int yy = y0 + y, xx = x0 + x;
        Px g = {};
        if (yy >= 0 && yy < Hs && xx >= 0 && xx < Ws) g = tap(yy, xx, r1);
#pragma unroll
        for (int c = 0; c < C; ++c)
            p1[((size_t)b * C + c) * pp + pix] = standardise(g.c[c], mean, inv_std);
    }
    // patch_2(x) = image(origin + Hpatch.x), bilinear, zeros outside (cv2.warpPerspective(img, inv(H)), utils.py:61-64)
    {
        const double* H = Hp + (size_t)b * 9;
        const double fx = x, fy = y;
        const double qz = H[6] * fx + H[7] * fy + H[8];
        const double wx = (H[0] * fx + H[1] * fy + H[2]) / qz, wy = (H[3] * fx + H[4] * fy + H[5]) / qz;
        if constexpr (TGT) {    // pf(x) = Hpatch.x - x (transforms.py:635-685), in double from the warp's own coordinate
            target[((size_t)b * 2) * pp + pix] = (float)(wx - fx);
            target[((size_t)b * 2 + 1) * pp + pix] = (float)(wy - fy);
        }
        const double u = wx + x0, v = wy + y0;
        const float uf = (float)u, vf = (float)v;
        const float xf = floorf(uf), yf = floorf(vf);
        const float ax = uf - xf, ay = vf - yf;
        Px g = {};
        auto add = [&](int yy, int xx, float kx, float ky) {
            const Px t = tap(yy, xx, r2);
#pragma unroll
            for (int c = 0; c < C; ++c) g.c[c] += t.c[c] * kx * ky;
        };
        if (xf >= -1.f && xf <= (float)Ws && yf >= -1.f && yf <= (float)Hs) {
            const int xi = (int)xf, yi = (int)yf;
            const bool vx0 = xi >= 0 && xi < Ws, vx1 = xi + 1 >= 0 && xi + 1 < Ws;
            const bool vy0 = yi >= 0 && yi < Hs, vy1 = yi + 1 >= 0 && yi + 1 < Hs;
            if (vx0 && vy0) add(yi, xi, 1 - ax, 1 - ay);
            if (vx1 && vy0) add(yi, xi + 1, ax, 1 - ay);
            if (vx0 && vy1) add(yi + 1, xi, 1 - ax, ay);
            if (vx1 && vy1) add(yi + 1, xi + 1, ax, ay);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) p2[((size_t)b * C + c) * pp + pix] = standardise(g.c[c], mean, inv_std);
    }
}

// image_1 of the photometric head's batch (config/s-coco/nguyen-orig-lr-5e-3.yaml: DictToGrayscale / DictStandardize also on 'image_1'):
// the whole base image under image 1's photometric record, grayscale, standardised - the plane patch_1 is cropped from, with the same
// per-pixel arithmetic as synth_pairs_kernel's patch_1 (its crop at `origin` equals patch_1 bitwise).  grid (ceil(Ws/16), ceil(Hs/16), B)
__global__ void __launch_bounds__(256) synth_image_kernel(const float* __restrict__ images, const int* __restrict__ img_idx,
                                                          const float* __restrict__ photo, int Hs, int Ws, float mean, float inv_std,
                                                          float* __restrict__ out) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= Ws || y >= Hs) return;
    const size_t plane = (size_t)Hs * Ws;
    const float* q = images + (size_t)img_idx[b] * 3 * plane + (size_t)y * Ws + x;
    float g;
    if (!photo) {
        g = q[0] * 0.299f + q[plane] * 0.587f + q[2 * plane] * 0.114f;                                  // transforms.py:351-353
    } else {
        const float* p = photo + (size_t)b * 12;                                                         // image 1's record
        const PhotoRec r1 = {p[0], p[1], p[2], p[3], p[4], (int)p[5]};
        g = photo_gray(q[0], q[plane], q[2 * plane], r1);
    }
    out[(size_t)b * plane + (size_t)y * Ws + x] = standardise(g, mean, inv_std);
}

extern "C" {

int bh_synth_image(const float* images, const int* img_idx, const float* photo, int B, int n_images, int Hs, int Ws, float mean,
                   float std, float* image1, void* stream) {
    if (!images || !img_idx || !image1 || B < 0 || n_images < 1 || Hs < 1 || Ws < 1 || std == 0.f) return BH_E_BADARG;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(synth_image_kernel, dim3((Ws + 15) / 16, (Hs + 15) / 16, B), dim3(256), 0, bh_stream(stream), images, img_idx,
                       photo, Hs, Ws, mean, 1.0f / std, image1);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_synth_batch(const float* images, const int* img_idx, const float* origin, const double* Hpatch, const float* photo,
                   int B, int n_images, int Hs, int Ws, int P, int C, float mean, float std, float* patch1, float* patch2,
                   float* target, void* stream) {
    if (!images || !img_idx || !origin || !Hpatch || !patch1 || !patch2 || B < 0 || n_images < 1 || std == 0.f || (C != 1 && C != 3))
        return BH_E_BADARG;
    if (P % 16) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(P / 16, P / 16, B), dim3(256), 0, bh_stream(stream), images, img_idx, origin, Hpatch, photo, Hs,
                           Ws, P, mean, 1.0f / std, patch1, patch2, target);
    };
    if (C == 1) target ? launch(synth_batch_kernel<1, true>) : launch(synth_batch_kernel<1, false>);
    else        target ? launch(synth_batch_kernel<3, true>) : launch(synth_batch_kernel<3, false>);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_synth_pairs(const float* images, const int* img_idx, const float* origin, const double* Hpatch, const float* photo,
                   int B, int n_images, int Hs, int Ws, int P, float mean, float std, float* patch1, float* patch2,
                   void* stream) {
    return bh_synth_batch(images, img_idx, origin, Hpatch, photo, B, n_images, Hs, Ws, P, 1, mean, std, patch1, patch2, nullptr, stream);
}

}  // extern "C"
