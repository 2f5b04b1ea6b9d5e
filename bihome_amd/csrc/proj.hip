// What a TRAINABLE projection head on top of the frozen perceptual features (AuxiliaryResnet WITH_PROJECTION_HEAD,
// src/heads/PerceptualHead.py:41-48,69-74) needs beyond the conv kernels that run its Linear layers:
//   bh_l2norm_fwd / _bwd        y = x / |x|_2 over the channels of a pixel (:470-479, :487-496) and its adjoint
//   bh_relu_bwd                 gx = gy [y > 0], the adjoint of the ReLU between two layers (:46-47)
//   bh_oneline_anchor_bwd       the gradient of the one-line loss (L1 / cosine) w.r.t. the UNWARPED maps f1, f2
//   bh_bihome_anchor_bwd        the same for the double-line loss (channel-agnostic / channel hinge)
// The adjoints in triplet.hip produce g_f1w / g_f2w only - f1 and f2 come from a frozen network there; with a projection on top they
// carry gradient into its weights.  These are separate launches: triplet.hip's kernels and their bits stay as they are.
// Layout as in triplet.hip: NHWC maps [.., hw, C], float4 per lane along the channels, LP = min(64, C / 4) lanes cooperate on a pixel and
// reduce with xor-shuffles, 64 / LP pixels per wave pass.  C: a multiple of 4 with C / 4 a divisor of 64 or at least 64 (else
// BH_E_UNSUPPORTED).  No atomics, no cross-workgroup sums: every output element has one writer and a fixed summation order - results are
// bitwise repeatable in every mode.  All launches go to the caller's stream, nothing synchronises the host.
// x / |x| has no epsilon, as upstream: a zero vector gives NaN (0 * inf) in y and in both gradients; nothing faults.
#include "common.h"
#include <initializer_list>

#define PROJ_COS_EPS 1e-8f                 // torch.cosine_similarity's, as triplet.hip
#define PROJ_BLOCKS_PER_SAMPLE 8
#define PROJ_MAX_BLOCKS 2048

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float sgn(float v) { return (v > 0.0f) ? 1.0f : ((v < 0.0f) ? -1.0f : 0.0f); }
__device__ __forceinline__ float4 sgn4(float4 a, float4 b) { return make_float4(sgn(a.x - b.x), sgn(a.y - b.y), sgn(a.z - b.z), sgn(a.w - b.w)); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
// the forward's hinge indicator of one channel (triplet.hip hinge1 / hinge_g): every pass sees the same expression
__device__ __forceinline__ float on1(float w, float o, float s, float margin) { return (fabsf(w - o) - fabsf(s - o) + margin > 0.0f) ? 1.0f : 0.0f; }
__device__ __forceinline__ float4 on4(float4 w, float4 o, float4 s, float m) {
    return make_float4(on1(w.x, o.x, s.x, m), on1(w.y, o.y, s.y, m), on1(w.z, o.z, s.z, m), on1(w.w, o.w, s.w, m));
}

// Lane geometry of a pixel walk over n pixels (block 256 = 4 waves): lane cl of LP works on pixel p0 + sub of a wave pass.  A lane whose
// pixel is past n, or whose channel group c0 + cl * 4 is past C, still takes part in the pass's shuffles: every loop below has the same
// trip count in all lanes of a wave.
struct Walk {
    int LP, sub, cl, first, stride, span;
    __device__ explicit Walk(int C) {
        LP = min(64, C / 4);
        const int PPW = 64 / LP;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        sub = lane / LP; cl = lane % LP;
        first = (blockIdx.x * 4 + wave) * PPW; stride = gridDim.x * 4 * PPW;
        span = LP * 4;                          // channels per pass over a pixel
    }
};

template <class... F>
__device__ __forceinline__ void lane_sum(int LP, F&... s) {
    for (int off = 1; off < LP; off <<= 1) ((s += __shfl_xor(s, off, 64)), ...);
}

// ---------------------------------------------------------------------------------------------
// y = x / |x|, inv = 1 / |x| per pixel;  gx = inv (g - y (y . g))
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) l2norm_fwd_kernel(const float* __restrict__ x, int M, int C, float* __restrict__ y,
                                                         float* __restrict__ inv) {
    const Walk w(C);
    for (int p0 = w.first; p0 < M; p0 += w.stride) {
        const int p = p0 + w.sub;
        const bool in = p < M;
        const size_t base = (size_t)p * C;
        float ss = 0.0f;
        for (int c0 = 0; c0 < C; c0 += w.span) {
            const int c = c0 + w.cl * 4;
            if (in && c < C) { const float4 v = ld4(x + base + c); ss += dot4(v, v); }
        }
        lane_sum(w.LP, ss);
        const float n = sqrtf(ss);
        for (int c0 = 0; c0 < C; c0 += w.span) {
            const int c = c0 + w.cl * 4;
            if (in && c < C) {
                const float4 v = ld4(x + base + c);
                st4(y + base + c, make_float4(v.x / n, v.y / n, v.z / n, v.w / n));       // (x / norm, as upstream writes it)
            }
        }
        if (in && w.cl == 0) inv[p] = 1.0f / n;
    }
}

__global__ void __launch_bounds__(256) l2norm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                         const float* __restrict__ inv, int M, int C, float* __restrict__ gx) {
    const Walk w(C);
    for (int p0 = w.first; p0 < M; p0 += w.stride) {
        const int p = p0 + w.sub;
        const bool in = p < M;
        const size_t base = (size_t)p * C;
        float d = 0.0f;
        for (int c0 = 0; c0 < C; c0 += w.span) {
            const int c = c0 + w.cl * 4;
            if (in && c < C) d += dot4(ld4(y + base + c), ld4(g + base + c));
        }
        lane_sum(w.LP, d);
        if (!in) continue;
        const float k = inv[p];
        for (int c = w.cl * 4; c < C; c += w.span) {
            const float4 a = ld4(g + base + c), b = ld4(y + base + c);
            st4(gx + base + c, make_float4(k * (a.x - b.x * d), k * (a.y - b.y * d), k * (a.z - b.z * d), k * (a.w - b.w * d)));
        }
    }
}

// gx = gy [y > 0] over n4 float4 groups
__global__ void __launch_bounds__(256) relu_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y, long long n4,
                                                       float* __restrict__ gx) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 g = ld4(gy + i * 4), v = ld4(y + i * 4);
        st4(gx + i * 4, make_float4(v.x > 0.0f ? g.x : 0.0f, v.y > 0.0f ? g.y : 0.0f, v.z > 0.0f ? g.z : 0.0f, v.w > 0.0f ? g.w : 0.0f));
    }
}

// ---------------------------------------------------------------------------------------------
// One line: t = d(f1w_q, f2; f1) + margin per hypothesis q = b rep + h;  k_q = [t > 0] g s_q m1w m2 / max(den_q, 1) - the expression of
// triplet_bwd_kernel.  Outputs per SAMPLE b, the hypotheses added in the order h = 0 .. rep - 1 inside the thread.
//   L1:      g_f1 = - sum_h k sgn(f1 - f2)                g_f2 = sum_h k (sgn(f1 - f2) - sgn(f1w_q - f2))
//   cosine:  g_f1 = sum_h k dc(f1, f2)/df1                g_f2 = sum_h k (dc(f1, f2)/df2 - dc(f1w_q, f2)/df2)
//            dc(x, o)/dx = o ix io - x (x.o ix io) ix / |x|,  ix = 1 / max(|x|, eps): the VALUE of a norm is clamped, its gradient is
//            not, and it is 0 at the zero vector (triplet.hip Cosine::Bwd)
// grid (PROJ_BLOCKS_PER_SAMPLE, samples), block 256.
// ---------------------------------------------------------------------------------------------
template <bool COS>
__global__ void __launch_bounds__(256) oneline_anchor_bwd_kernel(const float* __restrict__ g_loss, const float* __restrict__ f1,
                                                                 const float* __restrict__ f2, const float* __restrict__ f1w,
                                                                 const float* __restrict__ m1w, const float* __restrict__ m2,
                                                                 const float* __restrict__ T, const double* __restrict__ numden, int hw,
                                                                 int C, int rep, const float* __restrict__ sample_w,
                                                                 float* __restrict__ g_f1, float* __restrict__ g_f2) {
    const int b = blockIdx.y;
    const float g0 = g_loss[0];
    const Walk w(C);
    for (int p0 = w.first; p0 < hw; p0 += w.stride) {
        const int p = p0 + w.sub;
        const bool in = p < hw;
        const size_t qs = (size_t)b * hw + p, bases = qs * C;
        const float mm = (in && m2) ? m2[qs] : 1.0f;
        // cosine: the sums of the sample's own pair
        float d13 = 0.0f, n1 = 0.0f, n2 = 0.0f;
        if (COS) {
            for (int c0 = 0; c0 < C; c0 += w.span) {
                const int c = c0 + w.cl * 4;
                if (in && c < C) {
                    const float4 a1 = ld4(f1 + bases + c), a2 = ld4(f2 + bases + c);
                    d13 += dot4(a1, a2); n1 += dot4(a1, a1); n2 += dot4(a2, a2);
                }
            }
            lane_sum(w.LP, d13, n1, n2);
        }
        const float r1 = sqrtf(n1), r2 = sqrtf(n2);
        const float i1 = 1.0f / fmaxf(r1, PROJ_COS_EPS), i2 = 1.0f / fmaxf(r2, PROJ_COS_EPS);
        for (int c0 = 0; c0 < C; c0 += w.span) {
            const int c = c0 + w.cl * 4;
            const bool act = in && c < C;
            const float4 a1 = act ? ld4(f1 + bases + c) : zero4(), a2 = act ? ld4(f2 + bases + c) : zero4();
            const float4 s12 = sgn4(a1, a2);
            float4 o1 = zero4(), o2 = zero4();
            float K = 0.0f, S2 = 0.0f;             // cosine: sum_h k and sum_h k (f1w.f2 iw i2)
            for (int h = 0; h < rep; ++h) {
                const int q = b * rep + h;
                const size_t qp = (size_t)q * hw + p, base = qp * C;
                float k = 0.0f;
                if (in) {
                    const float g = g0 * (sample_w ? sample_w[q] : 1.0f);
                    const float den = fmaxf((float)numden[(size_t)q * 2 + 1], 1.0f);
                    k = T[qp] > 0.0f ? g * m1w[qp] * mm / den : 0.0f;
                }
                if (COS) {
                    float d1w = 0.0f, nw = 0.0f;
                    for (int e0 = 0; e0 < C; e0 += w.span) {
                        const int e = e0 + w.cl * 4;
                        if (in && e < C) {
                            const float4 aw = ld4(f1w + base + e), b2 = ld4(f2 + bases + e);
                            d1w += dot4(aw, b2); nw += dot4(aw, aw);
                        }
                    }
                    lane_sum(w.LP, d1w, nw);
                    const float iw = 1.0f / fmaxf(sqrtf(nw), PROJ_COS_EPS);
                    const float ka = k * iw * i2;                    // - k dc(f1w, f2)/df2 = - ka f1w + k (d1w iw i2) i2 / |f2| f2
                    K += k; S2 += k * (d1w * iw * i2);
                    if (act) {
                        const float4 aw = ld4(f1w + base + c);
                        o2.x -= ka * aw.x; o2.y -= ka * aw.y; o2.z -= ka * aw.z; o2.w -= ka * aw.w;
                    }
                } else if (act) {
                    const float4 sw = sgn4(ld4(f1w + base + c), a2);
                    o1.x -= k * s12.x; o1.y -= k * s12.y; o1.z -= k * s12.z; o1.w -= k * s12.w;
                    o2.x += k * (s12.x - sw.x); o2.y += k * (s12.y - sw.y); o2.z += k * (s12.z - sw.z); o2.w += k * (s12.w - sw.w);
                }
            }
            if (COS) {
                // K dc(f1, f2)/df1 and K dc(f1, f2)/df2 + the f2 term of the warped pairs
                const float c13 = d13 * i1 * i2;
                const float ka = K * i1 * i2;
                const float kb1 = (r1 > 0.0f) ? K * c13 * i1 / r1 : 0.0f;
                const float kb2 = (r2 > 0.0f) ? (K * c13 - S2) * i2 / r2 : 0.0f;
                o1 = make_float4(ka * a2.x - kb1 * a1.x, ka * a2.y - kb1 * a1.y, ka * a2.z - kb1 * a1.z, ka * a2.w - kb1 * a1.w);
                o2.x += ka * a1.x - kb2 * a2.x; o2.y += ka * a1.y - kb2 * a2.y; o2.z += ka * a1.z - kb2 * a2.z; o2.w += ka * a1.w - kb2 * a2.w;
            }
            if (act) { st4(g_f1 + bases + c, o1); st4(g_f2 + bases + c, o2); }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Two lines: elementwise, one scalar pair per pixel.  ka = g m1w m2 / max(den1, 1), kb = g m2w m1 / max(den2, 1) (m1 / m2 NULL = 1)
//   g_f1 = - ka I1 sgn(f1 - f2) - kb I2 (sgn(f2w - f1) + sgn(f1 - f2))      g_f2 = ka I1 (sgn(f1 - f2) - sgn(f1w - f2)) + kb I2 sgn(f1 - f2)
// I1 = I2 = 1 (channel-agnostic) or the forward's per-channel hinge indicators [|f1w - f2| - |f1 - f2| + margin > 0],
// [|f2w - f1| - |f1 - f2| + margin > 0].  One thread per float4 group of a pixel, grid-stride.
// ---------------------------------------------------------------------------------------------
template <bool HINGE>
__global__ void __launch_bounds__(256) bihome_anchor_bwd_kernel(const float* __restrict__ g_loss, const float* __restrict__ f1,
                                                                const float* __restrict__ f2, const float* __restrict__ f1w,
                                                                const float* __restrict__ f2w, const float* __restrict__ m1w,
                                                                const float* __restrict__ m2w, const float* __restrict__ m1,
                                                                const float* __restrict__ m2, const double* __restrict__ numden,
                                                                long long n4, int hw, int C4, float margin, float* __restrict__ g_f1,
                                                                float* __restrict__ g_f2) {
    const float g = g_loss[0];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long q = i / C4;                 // pixel (b, p)
        const long long b = q / hw;
        const float den1 = fmaxf((float)numden[b * 4 + 1], 1.0f), den2 = fmaxf((float)numden[b * 4 + 3], 1.0f);
        const float ka = g * m1w[q] * (m2 ? m2[q] : 1.0f) / den1, kb = g * m2w[q] * (m1 ? m1[q] : 1.0f) / den2;
        const float4 a1 = ld4(f1 + i * 4), a2 = ld4(f2 + i * 4), a1w = ld4(f1w + i * 4), a2w = ld4(f2w + i * 4);
        const float4 s12 = sgn4(a1, a2), s1w = sgn4(a1w, a2), s2w = sgn4(a2w, a1);
        float4 A = make_float4(ka, ka, ka, ka), Bk = make_float4(kb, kb, kb, kb);
        if (HINGE) {
            const float4 I1 = on4(a1w, a2, a1, margin), I2 = on4(a2w, a1, a2, margin);
            A = make_float4(ka * I1.x, ka * I1.y, ka * I1.z, ka * I1.w);
            Bk = make_float4(kb * I2.x, kb * I2.y, kb * I2.z, kb * I2.w);
        }
        st4(g_f1 + i * 4, make_float4(-A.x * s12.x - Bk.x * (s2w.x + s12.x), -A.y * s12.y - Bk.y * (s2w.y + s12.y),
                                      -A.z * s12.z - Bk.z * (s2w.z + s12.z), -A.w * s12.w - Bk.w * (s2w.w + s12.w)));
        st4(g_f2 + i * 4, make_float4(A.x * (s12.x - s1w.x) + Bk.x * s12.x, A.y * (s12.y - s1w.y) + Bk.y * s12.y,
                                      A.z * (s12.z - s1w.z) + Bk.z * s12.z, A.w * (s12.w - s1w.w) + Bk.w * s12.w));
    }
}

// the C set of the loss kernels (triplet.hip triplet_args)
int proj_args(std::initializer_list<const void*> need, long long rows, int C) {
    for (const void* p : need)
        if (!p) return BH_E_BADARG;
    if (rows < 0) return BH_E_BADARG;
    if (C % 4 || C < 4 || (C / 4 < 64 && (64 % (C / 4)))) return BH_E_UNSUPPORTED;
    return BH_OK;
}

int stream_blocks(long long items, int per_block) {
    const long long nb = (items + per_block - 1) / per_block;
    return (int)(nb < 1 ? 1 : (nb > PROJ_MAX_BLOCKS ? PROJ_MAX_BLOCKS : nb));
}

}  // namespace

extern "C" {

int bh_l2norm_fwd(const float* x, int M, int C, float* y, float* inv, void* stream) {
    if (int e = proj_args({x, y, inv}, M, C)) return e;
    if (M == 0) return BH_OK;
    const int ppb = 4 * (64 / (C / 4 < 64 ? C / 4 : 64));      // pixels per workgroup pass
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(stream_blocks(M, ppb)), dim3(256), 0, bh_stream(stream), x, M, C, y, inv);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_l2norm_bwd(const float* g, const float* y, const float* inv, int M, int C, float* gx, void* stream) {
    if (int e = proj_args({g, y, inv, gx}, M, C)) return e;
    if (M == 0) return BH_OK;
    const int ppb = 4 * (64 / (C / 4 < 64 ? C / 4 : 64));
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(stream_blocks(M, ppb)), dim3(256), 0, bh_stream(stream), g, y, inv, M, C, gx);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_relu_bwd(const float* gy, const float* y, long long n, float* gx, void* stream) {
    if (!gy || !y || !gx || n < 0 || n % 4) return BH_E_BADARG;
    if (n == 0) return BH_OK;
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(stream_blocks(n / 4, 256 * 4)), dim3(256), 0, bh_stream(stream), gy, y, n / 4, gx);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_oneline_anchor_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w, const float* m1w, const float* m2,
                          const float* T, const double* numden, int B, int hw, int C, int rep, const float* sample_w, int cosine,
                          float* g_f1, float* g_f2, void* stream) {
    if (int e = proj_args({g_loss, f1, f2, f1w, m1w, T, numden, g_f1, g_f2}, B, C)) return e;
    if (hw < 1 || rep < 1 || B % rep) return BH_E_BADARG;
    if (B / rep > 65535) return BH_E_UNSUPPORTED;               // (samples are gridDim.y)
    if (B == 0) return BH_OK;
    const dim3 grid(PROJ_BLOCKS_PER_SAMPLE, B / rep);
    if (cosine)
        hipLaunchKernelGGL(oneline_anchor_bwd_kernel<true>, grid, dim3(256), 0, bh_stream(stream), g_loss, f1, f2, f1w, m1w, m2, T, numden,
                           hw, C, rep, sample_w, g_f1, g_f2);
    else
        hipLaunchKernelGGL(oneline_anchor_bwd_kernel<false>, grid, dim3(256), 0, bh_stream(stream), g_loss, f1, f2, f1w, m1w, m2, T, numden,
                           hw, C, rep, sample_w, g_f1, g_f2);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_bihome_anchor_bwd(const float* g_loss, const float* f1, const float* f2, const float* f1w, const float* f2w, const float* m1w,
                         const float* m2w, const float* m1, const float* m2, const double* numden, int B, int hw, int C, float margin,
                         int hinge, float* g_f1, float* g_f2, void* stream) {
    if (int e = proj_args({g_loss, f1, f2, f1w, f2w, m1w, m2w, numden, g_f1, g_f2}, B, C)) return e;
    if (hw < 1) return BH_E_BADARG;
    if (B == 0) return BH_OK;
    const long long n4 = (long long)B * hw * (C / 4);
    const int blocks = stream_blocks(n4, 256 * 2);
    if (hinge)
        hipLaunchKernelGGL(bihome_anchor_bwd_kernel<true>, dim3(blocks), dim3(256), 0, bh_stream(stream), g_loss, f1, f2, f1w, f2w, m1w,
                           m2w, m1, m2, numden, n4, hw, C / 4, margin, g_f1, g_f2);
    else
        hipLaunchKernelGGL(bihome_anchor_bwd_kernel<false>, dim3(blocks), dim3(256), 0, bh_stream(stream), g_loss, f1, f2, f1w, f2w, m1w,
                           m2w, m1, m2, numden, n4, hw, C / 4, margin, g_f1, g_f2);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
