// Robust homography of a perspective field: batched RANSAC on the device (bh_ransac_homography, include/bihome.h) - what upstream's
// NoOpHead._postprocess does per sample on the host with cv2.findHomography(src, dst, cv2.RANSAC, 10) (src/heads/NoOpHead.py:75-109),
// with the minimal samples as an INPUT - and the Levenberg-Marquardt polish cv2 runs after its refit as a call of its own
// (bh_homography_refine_lm, at the end of this file).
//
//   ransac_hyp_kernel     one THREAD per (sample, hypothesis): the 8x8 solve of its four correspondences in double -> nine fp32
//                         coefficients (NaN for an invalid hypothesis) and count = 0 / -1
//   ransac_count_kernel   the hot one: a workgroup keeps 2048 correspondences of one sample in registers and walks all K hypotheses
//                         of that sample; the field is read once, cost grows with K through VALU work only
//   ransac_select_kernel  first hypothesis with the most inliers
//   ransac_sums_kernel    inlier mask of the winner + the Hartley statistics and the 24 sums of the normal matrix over ALL inliers
//   ransac_solve_kernel   9x9 Jacobi eigen-solve, denormalisation, corner transform - dlt_fwd_kernel's epilogue
//   homography_refine_lm_kernel   the polish: all Levenberg-Marquardt steps of a sample in one launch, one workgroup per sample
#include <math.h>
#include "geometry_dev.h"

// ---------------------------------------------------------------------------------------------
// The inlier test, shared by the counting kernel and the mask kernel so that both decide every pixel identically: the projective
// coordinates as fused multiply-adds in ONE order (the lesson of warp_tap.h), nothing left to the compiler's contraction.
// cv2's measure is (qx/qz - u)^2 + (qy/qz - v)^2 <= thr^2.  It is evaluated without the division, multiplied through by qz^2 > 0:
//     (qx - u qz)^2 + (qy - v qz)^2 <= (thr qz)^2
// - the same set in exact arithmetic, no reciprocal on the hot path, and both sides keep a relative rounding error of a few fp32 ulps
// however small qz is (the quotient form loses 1/qz^2 of that near the horizon of a wild hypothesis).  qz <= 0, infinite or NaN, or a
// NaN anywhere (an invalid hypothesis, a pixel beyond the end of the field) is an outlier.
// ---------------------------------------------------------------------------------------------
struct RansacH { float h0, h1, h2, h3, h4, h5, h6, h7, h8; };

__device__ __forceinline__ bool ransac_inlier(const RansacH& H, float x, float y, float u, float v, float thr) {
#pragma clang fp contract(off)
    const float qx = __builtin_fmaf(H.h0, x, __builtin_fmaf(H.h1, y, H.h2));
    const float qy = __builtin_fmaf(H.h3, x, __builtin_fmaf(H.h4, y, H.h5));
    const float qz = __builtin_fmaf(H.h6, x, __builtin_fmaf(H.h7, y, H.h8));
    const float a = __builtin_fmaf(-u, qz, qx), b = __builtin_fmaf(-v, qz, qy);
    const float e = __builtin_fmaf(b, b, a * a);
    const float t = thr * qz;
    return (qz > 0.0f) & (qz <= 3.402823466e38f) & (e <= t * t);      // (no short-circuit: straight-line code on the hot path)
}

// ---------------------------------------------------------------------------------------------
// Hypotheses.  grid ceil(B*K / 64), block 64; the 8x9 system of a thread lives in LDS (row stride 9, thread stride 73 doubles).
// Invalid (exact predicate, also in include/bihome.h):
//   - an index outside [0, h*w), or two equal indices;
//   - three collinear points among the four source or the four destination points: for every triple i < j < k, with
//     d1 = p_i - p_k, d2 = p_j - p_k:  |d2.x d1.y - d2.y d1.x| <= FLT_EPSILON (|d1.x| + |d1.y| + |d2.x| + |d2.y|)  (cv2's
//     haveCollinearPoints, in double, products and difference rounded separately);
//   - a pivot of the partial-pivoting elimination with |pivot| <= 1e-12 or NaN, or a non-finite coefficient.
// ---------------------------------------------------------------------------------------------
__device__ static bool collinear3(double xi, double yi, double xj, double yj, double xk, double yk) {
#pragma clang fp contract(off)
    const double dx1 = xi - xk, dy1 = yi - yk, dx2 = xj - xk, dy2 = yj - yk;
    const double p = dx2 * dy1, q = dy2 * dx1;
    return fabs(p - q) <= 1.1920928955078125e-07 * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

__device__ static bool any_collinear(const double* x, const double* y) {
    return collinear3(x[0], y[0], x[1], y[1], x[2], y[2]) || collinear3(x[0], y[0], x[1], y[1], x[3], y[3]) ||
           collinear3(x[0], y[0], x[2], y[2], x[3], y[3]) || collinear3(x[1], y[1], x[2], y[2], x[3], y[3]);
}

__global__ void __launch_bounds__(64) ransac_hyp_kernel(const float* __restrict__ pf, const int64_t* __restrict__ choice, int BK, int K,
                                                        int h, int w, float* __restrict__ hyp, int32_t* __restrict__ count) {
    __shared__ double sm[64 * 73];
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= BK) return;                                   // (no barrier below)
    const int b = t / K, N = h * w;
    const float* pfx = pf + (size_t)b * 2 * N;
    const float* pfy = pfx + N;
    double x[4], y[4], u[4], v[4];
    int64_t id[4];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        id[i] = choice[(size_t)t * 4 + i];
        const bool in = id[i] >= 0 && id[i] < (int64_t)N;
        ok = ok && in;
        const int p = in ? (int)id[i] : 0;                 // an index outside the field is never dereferenced
        x[i] = (double)(p % w); y[i] = (double)(p / w);
        u[i] = x[i] + (double)pfx[p]; v[i] = y[i] + (double)pfy[p];
    }
    ok = ok && id[0] != id[1] && id[0] != id[2] && id[0] != id[3] && id[1] != id[2] && id[1] != id[3] && id[2] != id[3];
    ok = ok && !any_collinear(x, y) && !any_collinear(u, v);
    double* S = sm + threadIdx.x * 73;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double* r0 = S + (2 * i) * 9;
        double* r1 = S + (2 * i + 1) * 9;
        r0[0] = x[i]; r0[1] = y[i]; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -x[i] * u[i]; r0[7] = -y[i] * u[i]; r0[8] = u[i];
        r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x[i]; r1[4] = y[i]; r1[5] = 1; r1[6] = -x[i] * v[i]; r1[7] = -y[i] * v[i]; r1[8] = v[i];
    }
    double hs[8];
    solve8(S, hs);
    for (int k = 0; k < 8; ++k) ok = ok && fabs(S[k * 9 + k]) > 1e-12 && fabs(hs[k]) <= 1.7976931348623157e308;      // (NaN fails both)
    const float nanf_ = __builtin_nanf("");
    for (int j = 0; j < 8; ++j) hyp[(size_t)t * 9 + j] = ok ? (float)hs[j] : nanf_;
    hyp[(size_t)t * 9 + 8] = ok ? 1.0f : nanf_;
    count[t] = ok ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------
// Inlier counting.  grid (ceil(h*w / 2048), B), block 256: thread `tid` keeps the correspondences of pixels tile*2048 + j*256 + tid,
// j < 8, in registers (a pixel beyond the field gets NaN destinations: never an inlier) and walks the K hypotheses of its sample.  The
// nine coefficients of a hypothesis are wave-uniform loads (scalar registers); per hypothesis a wave reduces its 8 x 64 decisions with
// ballot + popcount and lane 0 adds ONE integer into the workgroup's LDS table; at the end the table goes into count[B,K] with one
// integer atomic per hypothesis and workgroup (integer adds commute: the result does not depend on the arrival order).
// An invalid hypothesis is all NaN: it adds nothing and its count stays -1.
// ---------------------------------------------------------------------------------------------
#define RANSAC_PX 8
#define RANSAC_TILE (256 * RANSAC_PX)
#define RANSAC_KC 1024                      // hypotheses per pass of the LDS table

__global__ void __launch_bounds__(256) ransac_count_kernel(const float* __restrict__ pf, const float* __restrict__ hyp, int K, int h, int w,
                                                           float thr, int32_t* __restrict__ count) {
    __shared__ int s_cnt[RANSAC_KC];
    const int b = blockIdx.y, N = h * w, tid = threadIdx.x;
    const float* pfx = pf + (size_t)b * 2 * N;
    const float* pfy = pfx + N;
    float x[RANSAC_PX], y[RANSAC_PX], u[RANSAC_PX], v[RANSAC_PX];
#pragma unroll
    for (int j = 0; j < RANSAC_PX; ++j) {
        const int i = blockIdx.x * RANSAC_TILE + j * 256 + tid;
        const bool in = i < N;
        const int p = in ? i : 0;
        x[j] = (float)(p % w); y[j] = (float)(p / w);
        u[j] = in ? x[j] + pfx[p] : __builtin_nanf("");
        v[j] = in ? y[j] + pfy[p] : __builtin_nanf("");
    }
    const float* Hb = hyp + (size_t)b * K * 9;
    for (int k0 = 0; k0 < K; k0 += RANSAC_KC) {
        const int kn = min(RANSAC_KC, K - k0);
        for (int k = tid; k < kn; k += 256) s_cnt[k] = 0;
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            const float* Hm = Hb + (size_t)(k0 + k) * 9;
            const RansacH H = {Hm[0], Hm[1], Hm[2], Hm[3], Hm[4], Hm[5], Hm[6], Hm[7], Hm[8]};
            int c = 0;
#pragma unroll
            for (int j = 0; j < RANSAC_PX; ++j) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(ransac_inlier(H, x[j], y[j], u[j], v[j], thr)));
            if ((tid & 63) == 0 && c) atomicAdd(&s_cnt[k], c);
        }
        __syncthreads();
        for (int k = tid; k < kn; k += 256) {
            const int c = s_cnt[k];
            if (c) atomicAdd(count + (size_t)b * K + k0 + k, c);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Selection.  grid B, block 64: best[b] = the FIRST k with the maximal count (cv2 replaces its model only on strictly more inliers);
// n_inl[b] = that count, or 0 when it is below 4 (every hypothesis invalid, or nothing to refit on): the flag of the fallback.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) ransac_select_kernel(const int32_t* __restrict__ count, int K, int64_t* __restrict__ best,
                                                           int32_t* __restrict__ n_inl) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int bc = -2, bk = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const int c = count[(size_t)b * K + k];
        if (c > bc) { bc = c; bk = k; }                    // (ascending k per lane: the first maximum stays)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int oc = __shfl_xor(bc, off, 64), ok = __shfl_xor(bk, off, 64);
        if (oc > bc || (oc == bc && ok < bk)) { bc = oc; bk = ok; }
    }
    if (lane == 0) {
        best[b] = bk;
        n_inl[b] = bc >= 4 ? bc : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// Mask + sums of the refit.  grid B, block 1024: three sweeps over the sample's field (128 KB at 128 x 128: it stays in L2) - the
// means of the inlier coordinates (and the mask), their mean distances from the means (Hartley's scale needs the means first), then the
// 24 sums of the normal matrix (dlt_accumulate) - each reduced over the workgroup in a fixed order: no atomics, repeatable bits.
// A flagged sample (n_inl = 0) takes every point: mask all ones, the plain least-squares fit.
// work[b*32 ..]: 24 sums, then mx, my, s of the source and of the destination points.
// ---------------------------------------------------------------------------------------------
#define RANSAC_SUMS_THREADS 1024

template <int N>
__device__ __forceinline__ void block_sum(double* v, double* lds) {
    const int wave = threadIdx.x >> 6, nw = RANSAC_SUMS_THREADS / 64;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();                                       // the previous round's readers are done with lds
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds[wave * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double t = 0;
        for (int q = 0; q < nw; ++q) t += lds[q * N + i];
        v[i] = t;
    }
}

__global__ void __launch_bounds__(RANSAC_SUMS_THREADS) ransac_sums_kernel(const float* __restrict__ pf, const float* __restrict__ hyp,
                                                                          const int64_t* __restrict__ best, const int32_t* __restrict__ n_inl,
                                                                          int K, int h, int w, float thr, uint8_t* __restrict__ mask,
                                                                          double* __restrict__ work) {
    __shared__ double lds[(RANSAC_SUMS_THREADS / 64) * 24];
    const int b = blockIdx.x, N = h * w, tid = threadIdx.x;
    const float* pfx = pf + (size_t)b * 2 * N;
    const float* pfy = pfx + N;
    const bool all = n_inl[b] == 0;
    const float* Hm = hyp + ((size_t)b * K + (size_t)best[b]) * 9;
    const RansacH H = {Hm[0], Hm[1], Hm[2], Hm[3], Hm[4], Hm[5], Hm[6], Hm[7], Hm[8]};

    double s[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += RANSAC_SUMS_THREADS) {
        const float xf = (float)(i % w), yf = (float)(i / w), dx = pfx[i], dy = pfy[i];
        const bool in = all || ransac_inlier(H, xf, yf, xf + dx, yf + dy, thr);
        if (mask) mask[(size_t)b * N + i] = in ? 1 : 0;
        if (in) {
            const double x1 = (double)(i % w), y1 = (double)(i / w);
            s[0] += 1.0; s[1] += x1; s[2] += y1; s[3] += x1 + (double)dx; s[4] += y1 + (double)dy;
        }
    }
    block_sum<5>(s, lds);
    const double n = s[0] > 0 ? s[0] : 1.0;
    Hartley t1, t2;
    t1.mx = s[1] / n; t1.my = s[2] / n; t2.mx = s[3] / n; t2.my = s[4] / n;

    double d[2] = {0, 0};
    for (int i = tid; i < N; i += RANSAC_SUMS_THREADS) {
        const float xf = (float)(i % w), yf = (float)(i / w), dx = pfx[i], dy = pfy[i];
        if (all || ransac_inlier(H, xf, yf, xf + dx, yf + dy, thr)) {
            const double x1 = (double)(i % w), y1 = (double)(i / w), x2 = x1 + (double)dx, y2 = y1 + (double)dy;
            const double ax = x1 - t1.mx, ay = y1 - t1.my, bx = x2 - t2.mx, by = y2 - t2.my;
            d[0] += sqrt(ax * ax + ay * ay); d[1] += sqrt(bx * bx + by * by);
        }
    }
    block_sum<2>(d, lds);
    t1.dbar = d[0] / n; t2.dbar = d[1] / n;
    t1.s = 1.4142135623730951 / (t1.dbar + 1e-8); t2.s = 1.4142135623730951 / (t2.dbar + 1e-8);

    double acc[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i] = 0;
    for (int i = tid; i < N; i += RANSAC_SUMS_THREADS) {
        const float xf = (float)(i % w), yf = (float)(i / w), dx = pfx[i], dy = pfy[i];
        if (all || ransac_inlier(H, xf, yf, xf + dx, yf + dy, thr)) {
            const double x1 = (double)(i % w), y1 = (double)(i / w);
            dlt_accumulate(acc, t1, t2, x1, y1, x1 + (double)dx, y1 + (double)dy);
        }
    }
    block_sum<24>(acc, lds);
    double* wk = work + (size_t)b * 32;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 24; ++i) wk[i] = acc[i];
        wk[24] = t1.mx; wk[25] = t1.my; wk[26] = t1.s;
        wk[27] = t2.mx; wk[28] = t2.my; wk[29] = t2.s;
    }
}

// grid B, block 64 (jacobi9 is a one-wave routine)
__global__ void __launch_bounds__(64) ransac_solve_kernel(const double* __restrict__ work, int h, int w, float* __restrict__ Hout,
                                                          float* __restrict__ delta_hat) {
    __shared__ double A[81];
    __shared__ double V[81];
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* wk = work + (size_t)b * 32;
    if (lane == 0) dlt_normal_matrix(A, wk);
    __syncthreads();
    jacobi9(A, V, lane);
    if (lane == 0) {
        Hartley t1, t2;
        t1.mx = wk[24]; t1.my = wk[25]; t1.s = wk[26]; t1.dbar = 0;
        t2.mx = wk[27]; t2.my = wk[28]; t2.s = wk[29]; t2.dbar = 0;
        dlt_epilogue(A, V, t1, t2, w, h, Hout + (size_t)b * 9, delta_hat + (size_t)b * 8);
    }
}


// ---------------------------------------------------------------------------------------------
// Levenberg-Marquardt polish (bh_homography_refine_lm; the specification is in include/bihome.h).  grid B, block 512, ONE launch for
// all steps: pass 0 evaluates the start, pass it >= 1 the trial of step it - each pass is one sweep over the sample's field (it stays
// in L2: 128 KB at 128 x 128; the next pixel's three loads are issued before the current pixel's arithmetic), a fixed-order workgroup
// reduction of LM_NS sums in double, and the accept / reject decision + the damped 8x8 solve of the next step by thread 0.  No early
// exit: every sample runs iters + 1 passes whatever it decides, and a sample that is not (or no longer) live re-evaluates its own
// parameters.  512 threads, not the 1024 of ransac_sums_kernel: the 30 double accumulators and the temporaries of the division want
// ~170 vector registers, and a 1024-thread workgroup leaves 128 per thread (it spilled); 8 waves per CU keep no scratch.
//
// The sums.  With a = (x, y, 1) / qz and p = (qx, qy) / qz the two rows of the Jacobian of a correspondence are
//     d rx / d h = [a0 a1 a2  0  0  0  -a0 px  -a1 px],    d ry / d h = [ 0  0  0 a0 a1 a2  -a0 py  -a1 py]
// so the 36 unique entries of J^T J are 19 distinct sums (a a^T: 6, px a a^T and py a a^T without their last column: 5 each,
// (px^2 + py^2) a a^T without its last row and column: 3); with the 8 of J^T r, the cost, the number of correspondences and the number
// of them with qz <= 0 that is LM_NS = 30.
// ---------------------------------------------------------------------------------------------
#define LM_THREADS 512
#define LM_NS 30
#define LM_COST 0
#define LM_N 1
#define LM_BAD 2
#define LM_AA 3        // a0a0 a0a1 a0a2 a1a1 a1a2 a2a2
#define LM_X 9         // px * (a0a0 a0a1 a1a1 a2a0 a2a1)
#define LM_Y 14        // py * (the same)
#define LM_R 19        // (px^2 + py^2) * (a0a0 a0a1 a1a1)
#define LM_G 22        // J^T r

__device__ __forceinline__ bool lm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (NaN fails)

// a workgroup-uniform double into scalar registers: the eight parameters stay out of the vector register budget of the sweep
__device__ __forceinline__ double lm_uniform(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ void lm_accumulate(double* s, const double* __restrict__ par, double x, double y, double u, double v) {
    const double qx = par[0] * x + par[1] * y + par[2], qy = par[3] * x + par[4] * y + par[5], qz = par[6] * x + par[7] * y + 1.0;
    const double iz = 1.0 / qz;
    const double px = qx * iz, py = qy * iz, rx = px - u, ry = py - v;
    const double a0 = x * iz, a1 = y * iz, a2 = iz;
    const double a00 = a0 * a0, a01 = a0 * a1, a11 = a1 * a1, a20 = a2 * a0, a21 = a2 * a1;
    s[LM_COST] += rx * rx + ry * ry;
    s[LM_N] += 1.0;
    s[LM_BAD] += qz > 0.0 ? 0.0 : 1.0;                    // (a NaN qz counts)
    s[LM_AA] += a00; s[LM_AA + 1] += a01; s[LM_AA + 2] += a20; s[LM_AA + 3] += a11; s[LM_AA + 4] += a21; s[LM_AA + 5] += a2 * a2;
    s[LM_X] += px * a00; s[LM_X + 1] += px * a01; s[LM_X + 2] += px * a11; s[LM_X + 3] += px * a20; s[LM_X + 4] += px * a21;
    s[LM_Y] += py * a00; s[LM_Y + 1] += py * a01; s[LM_Y + 2] += py * a11; s[LM_Y + 3] += py * a20; s[LM_Y + 4] += py * a21;
    const double rr = px * px + py * py, pr = px * rx + py * ry;
    s[LM_R] += rr * a00; s[LM_R + 1] += rr * a01; s[LM_R + 2] += rr * a11;
    s[LM_G] += a0 * rx; s[LM_G + 1] += a1 * rx; s[LM_G + 2] += a2 * rx;
    s[LM_G + 3] += a0 * ry; s[LM_G + 4] += a1 * ry; s[LM_G + 5] += a2 * ry;
    s[LM_G + 6] -= a0 * pr; s[LM_G + 7] -= a1 * pr;
}

// (J^T J + lambda diag(J^T J)) d = -J^T r as the 8x9 augmented system of solve8; one lane
__device__ static void lm_system(double* S, const double* c, double lambda) {
    const int sym3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    const int xy[3][2] = {{0, 1}, {1, 2}, {3, 4}};
    const int sym2[2][2] = {{0, 1}, {1, 2}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            S[i * 9 + j] = c[LM_AA + sym3[i][j]]; S[(3 + i) * 9 + 3 + j] = c[LM_AA + sym3[i][j]];
            S[i * 9 + 3 + j] = 0; S[(3 + i) * 9 + j] = 0;
        }
        for (int j = 0; j < 2; ++j) {
            S[i * 9 + 6 + j] = -c[LM_X + xy[i][j]]; S[(6 + j) * 9 + i] = -c[LM_X + xy[i][j]];
            S[(3 + i) * 9 + 6 + j] = -c[LM_Y + xy[i][j]]; S[(6 + j) * 9 + 3 + i] = -c[LM_Y + xy[i][j]];
        }
    }
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) S[(6 + i) * 9 + 6 + j] = c[LM_R + sym2[i][j]];
    for (int i = 0; i < 8; ++i) {
        S[i * 9 + i] += lambda * S[i * 9 + i];
        S[i * 9 + 8] = -c[LM_G + i];
    }
}

__global__ void __launch_bounds__(LM_THREADS) homography_refine_lm_kernel(const float* __restrict__ pf, const uint8_t* __restrict__ mask,
                                                                          int h, int w, int iters, float* __restrict__ H,
                                                                          float* __restrict__ delta_hat, double* __restrict__ work) {
    __shared__ double red[(LM_THREADS / 64) * LM_NS];
    __shared__ double cur[LM_NS];          // the sums at the current parameters
    __shared__ double S[72];
    __shared__ double par[8];              // what the next pass evaluates: the start, then the trial of every step
    __shared__ double pc[8];               // the current parameters
    __shared__ double dstep[8];            // thread 0: the step of the solve
    __shared__ double st[2];               // thread 0: lambda, the start's cost
    __shared__ int fl[4];                  // thread 0: accepted steps, live, stepped, failed
    const int b = blockIdx.x, N = h * w, tid = threadIdx.x;
    const float* pfx = pf + (size_t)b * 2 * N;
    const float* pfy = pfx + N;
    const uint8_t* mk = mask ? mask + (size_t)b * N : nullptr;
    float* Hb = H + (size_t)b * 9;
    const int x0 = tid % w, y0 = tid / w, sx = LM_THREADS % w, sy = LM_THREADS / w;
    if (tid == 0) {
        const double h8 = (double)Hb[8];
        for (int k = 0; k < 8; ++k) par[k] = pc[k] = (double)Hb[k] / h8;
        st[0] = 1e-3; st[1] = 0.0;
        fl[0] = fl[1] = fl[2] = fl[3] = 0;
    }
    __syncthreads();

    for (int it = 0; it <= iters; ++it) {
        double s[LM_NS];
#pragma unroll
        for (int i = 0; i < LM_NS; ++i) s[i] = 0.0;
        {
            double p[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k] = lm_uniform(par[k]);
            int i = tid, x = x0, y = y0;
            bool in = false;
            float dx = 0.0f, dy = 0.0f;
            if (i < N) { in = mk ? mk[i] != 0 : true; dx = pfx[i]; dy = pfy[i]; }
            while (i < N) {
                const int i2 = i + LM_THREADS;
                bool in2 = false;
                float dx2 = 0.0f, dy2 = 0.0f;
                if (i2 < N) { in2 = mk ? mk[i2] != 0 : true; dx2 = pfx[i2]; dy2 = pfy[i2]; }
                if (in) lm_accumulate(s, p, (double)x, (double)y, (double)x + (double)dx, (double)y + (double)dy);
                i = i2; in = in2; dx = dx2; dy = dy2;
                x += sx; y += sy;
                if (x >= w) { x -= w; ++y; }
            }
        }
        // fixed order: the pixels of a thread in ascending order, the butterfly of a wave, then the 8 waves in order (thread 0)
#pragma unroll
        for (int i = 0; i < LM_NS; ++i) s[i] = wave_sum(s[i]);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int i = 0; i < LM_NS; ++i) red[(tid >> 6) * LM_NS + i] = s[i];
        }
        __syncthreads();
        if (tid == 0) {                                    // (its state lives in LDS, not in registers the sweep would have to carry)
            int accepted = fl[0];
            bool live = fl[1] != 0, stepped = fl[2] != 0, failed = fl[3] != 0;
            for (int i = 0; i < LM_NS; ++i) {
                double t = 0;
                for (int q = 0; q < LM_THREADS / 64; ++q) t += red[q * LM_NS + i];
                S[i] = t;                                   // (S is free until lm_system)
            }
            const bool good = S[LM_BAD] == 0.0 && lm_finite(S[LM_COST]);
            if (it == 0) {
                st[1] = S[LM_COST];
                live = good && S[LM_N] >= 4.0;
                for (int k = 0; k < 8; ++k) live = live && lm_finite(pc[k]);
                for (int i = 0; i < LM_NS; ++i) cur[i] = S[i];
            } else if (stepped) {
                if (good && S[LM_COST] < cur[LM_COST]) {
                    for (int k = 0; k < 8; ++k) pc[k] = par[k];
                    for (int i = 0; i < LM_NS; ++i) cur[i] = S[i];
                    st[0] = fmax(st[0] / 10.0, 1e-12);
                    ++accepted;
                } else {
                    st[0] = fmin(st[0] * 10.0, 1e12);
                }
            }
            stepped = false;
            if (live && it < iters) {
                double* d = dstep;
                lm_system(S, cur, st[0]);
                solve8(S, d);
                bool ok = true;
                for (int k = 0; k < 8; ++k) ok = ok && fabs(S[k * 9 + k]) > 1e-12 && lm_finite(d[k]);      // ransac_hyp_kernel's rule
                if (ok) {
                    for (int k = 0; k < 8; ++k) par[k] = pc[k] + d[k];
                    stepped = true;
                } else {
                    live = false; failed = true;
                }
            }
            if (!stepped)
                for (int k = 0; k < 8; ++k) par[k] = pc[k];
            fl[0] = accepted; fl[1] = live; fl[2] = stepped; fl[3] = failed;
        }
        __syncthreads();
    }

    if (tid == 0) {
        double cost1 = cur[LM_COST];
        int accepted = fl[0];
        if (fl[3]) {                                      // a failed solve: the sample keeps its START
            const double h8 = (double)Hb[8];
            for (int k = 0; k < 8; ++k) pc[k] = (double)Hb[k] / h8;
            accepted = 0; cost1 = st[1];
        }
        if (accepted > 0) {                                // (no accepted step: H stays as it was passed in)
            for (int k = 0; k < 8; ++k) Hb[k] = (float)pc[k];
            Hb[8] = 1.0f;
        }
        float* dh = delta_hat + (size_t)b * 8;
        for (int c = 0; c < 4; ++c) {                      // dlt_epilogue's corner transform
            double x, y;
            corner_xy(c, (double)w, (double)h, x, y);
            const double qx = pc[0] * x + pc[1] * y + pc[2], qy = pc[3] * x + pc[4] * y + pc[5], qz = pc[6] * x + pc[7] * y + 1.0;
            const double sc = fabs(qz) > 1e-8 ? 1.0 / qz : 1.0;
            dh[2 * c] = (float)(qx * sc - x);
            dh[2 * c + 1] = (float)(qy * sc - y);
        }
        double* wk = work + (size_t)b * 4;
        wk[0] = st[1]; wk[1] = cost1; wk[2] = (double)accepted; wk[3] = st[0];
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" {

int bh_ransac_homography(const float* pf, const int64_t* choice, int B, int K, int h, int w, float thr, float* hyp, int32_t* count,
                         int64_t* best, int32_t* n_inl, uint8_t* mask, double* work, float* H, float* delta_hat, void* stream) {
    if (!pf || !choice || !hyp || !count || !best || !n_inl || !work || !H || !delta_hat) return BH_E_BADARG;
    if (B < 0 || K < 1 || h < 1 || w < 1 || (long long)h * w < 4 || !(thr >= 0.0f)) return BH_E_BADARG;
    if ((long long)h * w > (1ll << 30) || (long long)B * K > (1ll << 30) || B > 65535) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    hipStream_t st = bh_stream(stream);
    const int BK = B * K, N = h * w;
    hipLaunchKernelGGL(ransac_hyp_kernel, dim3((BK + 63) / 64), dim3(64), 0, st, pf, choice, BK, K, h, w, hyp, count);
    BH_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_count_kernel, dim3((N + RANSAC_TILE - 1) / RANSAC_TILE, B), dim3(256), 0, st, pf, hyp, K, h, w, thr, count);
    BH_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_select_kernel, dim3(B), dim3(64), 0, st, count, K, best, n_inl);
    BH_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_sums_kernel, dim3(B), dim3(RANSAC_SUMS_THREADS), 0, st, pf, hyp, best, n_inl, K, h, w, thr, mask, work);
    BH_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_solve_kernel, dim3(B), dim3(64), 0, st, work, h, w, H, delta_hat);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_homography_refine_lm(const float* pf, const uint8_t* mask, int B, int h, int w, int iters, float* H, float* delta_hat, double* work,
                            void* stream) {
    if (!pf || !H || !delta_hat || !work) return BH_E_BADARG;
    if (B < 0 || h < 1 || w < 1 || (long long)h * w < 4 || iters < 0) return BH_E_BADARG;
    if ((long long)h * w > (1ll << 30) || B > 65535) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(homography_refine_lm_kernel, dim3(B), dim3(LM_THREADS), 0, bh_stream(stream), pf, mask, h, w, iters, H, delta_hat, work);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
