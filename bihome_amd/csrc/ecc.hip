// Coarse-to-fine ECC refinement of a homography on two image pyramids (include/bihome.h "ECC refinement"; bihome_amd/align.py holds the
// numpy float64 statements gray_pyramid_host / ecc_sums_host / ecc_step_host / ecc_refine_host the kernels are tested against).
//
// bh_gray_pyramid_u8: uint8 interleaved RGB (u8_image.h u8_image / ld_rgb_u8) -> gray float planes, level l the 2 x 2 box mean of level l - 1, one launch per level, one
// thread and one writer per element.  The gray value is two written-out fused multiply-adds, the box mean plain float operations without
// contraction: the bits of a float32 numpy restatement.
//
// bh_ecc_sums: one pass over image B's plane at one level.  A workgroup of 256 threads takes ECC_BLOCK_PIXELS consecutive pixels; a thread
// projects its pixel with warp_tap.h's tap_project / tap_place (the spelling bh_warp_u8 takes its taps with), forms z = (j0..j7, iw, t, 1)
// in float and adds the 66 products z_i z_j (i <= j) to float accumulators for ECC_PX pixels, then moves them into double accumulators;
// the workgroup's doubles are summed by a butterfly across the lanes and in wave order through LDS - one partial block of 66 doubles per
// workgroup, plain vector stores - and a second launch adds the partial blocks of a sample in block-index order.  No atomics anywhere:
// two calls give equal bits.
//
// bh_ecc_step: one workgroup per sample.  80 threads own one element each of the 8 x 10 augmented system [G'^T G' | a  c] in LDS and
// eliminate with partial pivoting (every thread finds the pivot from the same column, so the choice is uniform), thread 0 substitutes back
// and keeps the books (best so far, frozen, counters, the change of level).  Double, and without contraction: the operations of
// ecc_step_host in its order.
//
// bh_ecc_refine: the whole schedule on one stream - per level iters + 1 times (sums, partial reduction + step in one launch).
#include "u8_image.h"

#define ECC_THREADS 256
#define ECC_PX 16                                       // pixels a float accumulator carries before it is added to a double
#define ECC_ROUNDS 4
#define ECC_BLOCK_PIXELS (ECC_THREADS * ECC_PX * ECC_ROUNDS)
#define ECC_NZ 11
#define ECC_NS BH_ECC_SUMS
#define ECC_STEP_THREADS 128
#define ECC_MAX_LEVELS 6
#define ECC_MIN_SIDE 8

static_assert(ECC_NS == ECC_NZ * (ECC_NZ + 1) / 2, "the upper triangle of z z^T");

// index of entry (i, j), i <= j, of the row-major upper triangle of the 11 x 11 Gram matrix (include/bihome.h)
__host__ __device__ constexpr int ecc_at(int i, int j) { return i * ECC_NZ - i * (i - 1) / 2 + (j - i); }

// ------------------------------------------------------------------------------------------------
// the pyramid
// ------------------------------------------------------------------------------------------------
// grid (ceil(H * W / ECC_THREADS), u8_grid_y(B)); H * W >= 64
__global__ void __launch_bounds__(ECC_THREADS) ecc_gray_kernel(const unsigned char* __restrict__ images, const int* __restrict__ idx, int n_images,
                                                               int H, int W, int B, size_t total, float* __restrict__ pyr) {
#pragma clang fp contract(off)
    const unsigned n = (unsigned)H * (unsigned)W;
    const unsigned u = blockIdx.x * ECC_THREADS + threadIdx.x;
    if (u >= n) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const unsigned v = ld_rgb_u8<false>(u8_image(images, idx, b, n_images, n), u);
        const float r = (float)(v & 255u), g = (float)((v >> 8) & 255u), bl = (float)((v >> 16) & 255u);
        pyr[(size_t)b * total + u] = __builtin_fmaf(0.114f, bl, __builtin_fmaf(0.587f, g, 0.299f * r));
    }
}

// level l from level l - 1 (hs x ws at `from`, hd x wd at `to`, both inside a sample's row of `total` floats)
__global__ void __launch_bounds__(ECC_THREADS) ecc_halve_kernel(float* __restrict__ pyr, size_t total, size_t from, int ws, size_t to, int hd, int wd, int B) {
#pragma clang fp contract(off)
    const unsigned u = blockIdx.x * ECC_THREADS + threadIdx.x;
    if (u >= (unsigned)hd * (unsigned)wd) return;
    const unsigned y = u / (unsigned)wd, x = u - y * (unsigned)wd;
    const size_t o = (size_t)(2u * y) * (unsigned)ws + 2u * x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ s = pyr + (size_t)b * total + from;
        const float a = s[o], c = s[o + 1], d = s[o + (unsigned)ws], e = s[o + (unsigned)ws + 1];
        pyr[(size_t)b * total + to + u] = ((a + c) + (d + e)) * 0.25f;
    }
}

// ------------------------------------------------------------------------------------------------
// one pass
// ------------------------------------------------------------------------------------------------
// H / H[8] as floats (the division in double; exact and without effect for H[8] = 1, which is what the refinement keeps)
__device__ __forceinline__ Hf ecc_load_h(const double* __restrict__ Hm) {
    const double s = Hm[8];
    Hf f;
    f.h0 = (float)(Hm[0] / s); f.h1 = (float)(Hm[1] / s); f.h2 = (float)(Hm[2] / s); f.h3 = (float)(Hm[3] / s); f.h4 = (float)(Hm[4] / s);
    f.h5 = (float)(Hm[5] / s); f.h6 = (float)(Hm[6] / s); f.h7 = (float)(Hm[7] / s); f.h8 = (float)(s / s);
    return f;
}

// z = (j0..j7, iw, t, 1) of pixel (x, y) of T, all zeros where the pixel does not count
__device__ __forceinline__ void ecc_pixel(const float* __restrict__ A, int Wa, int Ha, const Hf& Hm, int x, int y, float tv, bool on, float (&z)[ECC_NZ]) {
#pragma clang fp contract(off)
    const Tap4 t = make_tap4(Hm, x, y, Wa, Ha);
    // counts: qz > 1e-8 (the guard is |qz| <= 1e-8; iz has qz's sign), all four taps inside A, the mask byte (and the pixel exists)
    const bool c = on && !t.guard && t.iz > 0.0f && t.vx0 && t.vx1 && t.vy0 && t.vy1;
    const unsigned o = c ? (t.o00 >> 2) : 0u;
    const unsigned right = c ? 1u : 0u, down = c ? (unsigned)Wa : 0u;
    const float a00 = A[o], a01 = A[o + right], a10 = A[o + down], a11 = A[o + down + right];
    float w00, w01, w10, w11, wsum;
    tap_weights(t, w00, w01, w10, w11, wsum);
    const float iw = tap_blend(a00, a01, a10, a11, w00, w01, w10, w11);
    const float gx = __builtin_fmaf(t.fy, a11 - a10, (1.0f - t.fy) * (a01 - a00));
    const float gy = __builtin_fmaf(t.fx, a11 - a01, (1.0f - t.fx) * (a10 - a00));
    const float m = -__builtin_fmaf(gy, t.v, gx * t.u);
    const float xf = (float)x, yf = (float)y;
    const float gxz = gx * t.iz, gyz = gy * t.iz, mz = m * t.iz;
    z[0] = c ? gxz * xf : 0.0f; z[1] = c ? gxz * yf : 0.0f; z[2] = c ? gxz : 0.0f;
    z[3] = c ? gyz * xf : 0.0f; z[4] = c ? gyz * yf : 0.0f; z[5] = c ? gyz : 0.0f;
    z[6] = c ? mz * xf : 0.0f;  z[7] = c ? mz * yf : 0.0f;
    z[8] = c ? iw : 0.0f; z[9] = c ? tv : 0.0f; z[10] = c ? 1.0f : 0.0f;
}

// grid (ceil(Hb * Wb / ECC_BLOCK_PIXELS), u8_grid_y(B)); partial[B, gridDim.x, 66].  A thread's pixels lie ECC_THREADS apart, so
// (x, y) advances by (ECC_THREADS % Wb, ECC_THREADS / Wb) with one carry: one division per thread, none per pixel.
template <bool MASK>
__global__ void __launch_bounds__(ECC_THREADS) ecc_sums_kernel(const float* __restrict__ a, int Ha, int Wa, size_t a_stride, const float* __restrict__ t,
                                                               int Hb, int Wb, size_t t_stride, const unsigned char* __restrict__ mask, size_t m_stride,
                                                               const double* __restrict__ H64, int h_stride, int B, double* __restrict__ partial) {
    __shared__ double sm[ECC_THREADS / 64][ECC_NS];
    const unsigned npix = (unsigned)Hb * (unsigned)Wb;
    const unsigned base = blockIdx.x * (unsigned)ECC_BLOCK_PIXELS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned dx = (unsigned)ECC_THREADS % (unsigned)Wb, dy = (unsigned)ECC_THREADS / (unsigned)Wb;
    const unsigned y_first = base / (unsigned)Wb, x_first = base - y_first * (unsigned)Wb;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const Hf Hm = ecc_load_h(H64 + (size_t)b * h_stride);
        const float* __restrict__ A = a + (size_t)b * a_stride;
        const float* __restrict__ T = t + (size_t)b * t_stride;
        const unsigned char* __restrict__ M = MASK ? mask + (size_t)b * m_stride : nullptr;
        unsigned x = x_first, y = y_first;
        double dacc[ECC_NS];
#pragma unroll
        for (int k = 0; k < ECC_NS; ++k) dacc[k] = 0.0;
        for (int r = 0; r < ECC_ROUNDS; ++r) {
            const unsigned first = base + (unsigned)r * (ECC_THREADS * ECC_PX);
            if (first - threadIdx.x >= npix) break;                     // (uniform: the round lies behind the plane)
            float acc[ECC_NS];
#pragma unroll
            for (int k = 0; k < ECC_NS; ++k) acc[k] = 0.0f;
#pragma unroll 2
            for (int i = 0; i < ECC_PX; ++i) {
                const unsigned pix = first + (unsigned)i * ECC_THREADS;
                const bool in = pix < npix;
                const unsigned p = in ? pix : 0u;
                bool on = in;
                if constexpr (MASK) on = on && M[p] != 0;
                float z[ECC_NZ];
                ecc_pixel(A, Wa, Ha, Hm, (int)x, (int)y, T[p], on, z);
                x += dx; y += dy;
                if (x >= (unsigned)Wb) { x -= (unsigned)Wb; y += 1u; }
                int k = 0;
#pragma unroll
                for (int i0 = 0; i0 < ECC_NZ; ++i0)
#pragma unroll
                    for (int i1 = i0; i1 < ECC_NZ; ++i1, ++k) acc[k] = __builtin_fmaf(z[i0], z[i1], acc[k]);
            }
#pragma unroll
            for (int k = 0; k < ECC_NS; ++k) dacc[k] += (double)acc[k];
        }
#pragma unroll
        for (int k = 0; k < ECC_NS; ++k) {
            const double s = wave_sum(dacc[k]);
            if (lane == 0) sm[wave][k] = s;
        }
        __syncthreads();
        if (threadIdx.x < ECC_NS)
            partial[((size_t)b * gridDim.x + blockIdx.x) * ECC_NS + threadIdx.x] =
                ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
        __syncthreads();
    }
}

// grid B, block ECC_STEP_THREADS: sums[b, k] = the partial blocks of sample b added in block-index order
__global__ void __launch_bounds__(ECC_STEP_THREADS) ecc_reduce_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ sums) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= ECC_NS) return;
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += partial[((size_t)b * nblk + i) * ECC_NS + k];
    sums[(size_t)b * ECC_NS + k] = s;
}

// ------------------------------------------------------------------------------------------------
// one step
// ------------------------------------------------------------------------------------------------
// state[b] (BH_ECC_STATE doubles): 0..8 cur, 9..17 best, 18 rho_best, 19 frozen, 20 rho at the level's first pass, 21 accepted steps,
// 22 passes done at this level
#define ST_CUR 0
#define ST_BEST 9
#define ST_RHO_BEST 18
#define ST_FROZEN 19
#define ST_RHO_FIRST 20
#define ST_ACCEPTED 21
#define ST_PASSES 22

// H -> C H C^-1 (a level down, to the finer one) or C^-1 H C (a level up), C = [[2, 0, .5], [0, 2, .5], [0, 0, 1]], scaled to H[8] = 1
__device__ void ecc_change_level(double* H, bool down) {
    const double C[9] = {2.0, 0.0, 0.5, 0.0, 2.0, 0.5, 0.0, 0.0, 1.0}, Ci[9] = {0.5, 0.0, -0.25, 0.0, 0.5, -0.25, 0.0, 0.0, 1.0};
    double t[9], r[9];
    mat3_mul(down ? C : Ci, H, t);
    mat3_mul(t, down ? Ci : C, r);
    for (int i = 0; i < 9; ++i) H[i] = r[i] / r[8];
}

// grid B, block ECC_STEP_THREADS.  REDUCE: the sums are the partial blocks' (added here, in block-index order), else read from `sums`.
// last: 0 = a pass that may step; 1 = the level's last pass (the result, best, becomes cur; stats written); 2 = as 1, then cur moves a
// level down and the books are reset for it.  Hout (NULL ok): cur as this call leaves it.
template <bool REDUCE>
__global__ void __launch_bounds__(ECC_STEP_THREADS) ecc_step_kernel(const double* __restrict__ src, int nblk, double* __restrict__ state, int last,
                                                                    double* __restrict__ stats, int stats_stride, double* __restrict__ Hout) {
#pragma clang fp contract(off)
    __shared__ double S[ECC_NS];
    __shared__ double M[8][10];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < ECC_NS) {
        double s;
        if constexpr (REDUCE) {
            s = 0.0;
            for (int i = 0; i < nblk; ++i) s += src[((size_t)b * nblk + i) * ECC_NS + tid];
        } else {
            s = src[(size_t)b * ECC_NS + tid];
        }
        S[tid] = s;
    }
    __syncthreads();
    const double n = S[ecc_at(10, 10)];
    const double m_iw = S[ecc_at(8, 10)] / n, m_t = S[ecc_at(9, 10)] / n;
    const double v_iw = S[ecc_at(8, 8)] - (n * m_iw) * m_iw, v_t = S[ecc_at(9, 9)] - (n * m_t) * m_t;
    const double c_it = S[ecc_at(8, 9)] - (n * m_iw) * m_t;
    const bool measured = n >= 16.0 && v_iw > 0.0 && v_t > 0.0;
    const int r = tid / 10, c = tid - r * 10;
    if (tid < 80) {
        double v;
        if (c < 8) v = S[ecc_at(r < c ? r : c, r < c ? c : r)] - (S[ecc_at(r, 10)] * S[ecc_at(c, 10)]) / n;
        else if (c == 8) v = S[ecc_at(r, 8)] - m_iw * S[ecc_at(r, 10)];
        else v = S[ecc_at(r, 9)] - m_t * S[ecc_at(r, 10)];
        M[r][c] = v;
    }
    __syncthreads();
    bool solved = true;
    for (int k = 0; k < 8; ++k) {
        int p = k;
        double big = fabs(M[k][k]);
        for (int q = k + 1; q < 8; ++q) {
            const double v = fabs(M[q][k]);
            if (v > big) { big = v; p = q; }
        }
        if (!(big > 0.0)) solved = false;                               // a zero or NaN pivot (uniform: every thread read the same column)
        __syncthreads();
        if (p != k && tid < 10) {
            const double u = M[k][tid], w = M[p][tid];
            M[k][tid] = w; M[p][tid] = u;
        }
        __syncthreads();
        if (tid < 80 && r > k && c > k) {
            const double f = M[r][k] / M[k][k];
            M[r][c] = M[r][c] - f * M[k][c];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double* st = state + (size_t)b * BH_ECC_STATE;
    double ya[8], yc[8];
    for (int i = 7; i >= 0; --i) {
        double sa = M[i][8], sc = M[i][9];
        for (int j = i + 1; j < 8; ++j) { sa = sa - M[i][j] * ya[j]; sc = sc - M[i][j] * yc[j]; }
        ya[i] = sa / M[i][i]; yc[i] = sc / M[i][i];
    }
    // a and c once more (the elimination overwrote its copies)
    double da = 0.0, dc = 0.0;
    for (int i = 0; i < 8; ++i) {
        const double ai = S[ecc_at(i, 8)] - m_iw * S[ecc_at(i, 10)], ci = S[ecc_at(i, 9)] - m_t * S[ecc_at(i, 10)];
        da = da + ai * ya[i]; dc = dc + ci * ya[i];
    }
    const double lambda_n = v_iw - da, lambda_d = c_it - dc;
    double d[8];
    bool step_ok = measured && solved && lambda_d > 0.0;
    const double lambda = lambda_n / lambda_d;
    for (int i = 0; i < 8; ++i) {
        d[i] = lambda * yc[i] - ya[i];
        if (!(fabs(d[i]) < __builtin_inf())) step_ok = false;
    }
    const double rho = measured ? c_it / sqrt(v_iw * v_t) : __builtin_nan("");
    // the books
    if (st[ST_PASSES] == 0.0) st[ST_RHO_FIRST] = rho;
    st[ST_PASSES] = st[ST_PASSES] + 1.0;
    if (st[ST_FROZEN] == 0.0) {
        if (rho > st[ST_RHO_BEST]) {
            for (int i = 0; i < 9; ++i) st[ST_BEST + i] = st[ST_CUR + i];
            st[ST_RHO_BEST] = rho;
            if (last == 0 && step_ok) {
                for (int i = 0; i < 8; ++i) st[ST_CUR + i] = st[ST_CUR + i] + d[i];
                st[ST_CUR + 8] = 1.0;
                st[ST_ACCEPTED] = st[ST_ACCEPTED] + 1.0;
            } else {
                st[ST_FROZEN] = 1.0;
            }
        } else {
            for (int i = 0; i < 9; ++i) st[ST_CUR + i] = st[ST_BEST + i];
            st[ST_FROZEN] = 1.0;
        }
    }
    if (last != 0) {
        for (int i = 0; i < 9; ++i) st[ST_CUR + i] = st[ST_BEST + i];
        if (stats) {
            double* o = stats + (size_t)b * stats_stride;
            o[0] = st[ST_RHO_FIRST]; o[1] = st[ST_RHO_BEST]; o[2] = st[ST_ACCEPTED];
        }
        if (last == 2) {
            double Hm[9];
            for (int i = 0; i < 9; ++i) Hm[i] = st[ST_CUR + i];
            ecc_change_level(Hm, true);
            for (int i = 0; i < 9; ++i) { st[ST_CUR + i] = Hm[i]; st[ST_BEST + i] = Hm[i]; }
            st[ST_RHO_BEST] = -__builtin_inf(); st[ST_FROZEN] = 0.0; st[ST_RHO_FIRST] = 0.0; st[ST_ACCEPTED] = 0.0; st[ST_PASSES] = 0.0;
        }
    }
    if (Hout)
        for (int i = 0; i < 9; ++i) Hout[(size_t)b * 9 + i] = st[ST_CUR + i];
}

// grid ceil(B / 64), block 64: the start of a refinement - H64[b] / H64[b][8] taken `up` levels up, the books of a fresh level
__global__ void __launch_bounds__(64) ecc_start_kernel(const double* __restrict__ H64, int B, int up, double* __restrict__ state) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double Hm[9];
    for (int i = 0; i < 9; ++i) Hm[i] = H64[(size_t)b * 9 + i] / H64[(size_t)b * 9 + 8];
    for (int l = 0; l < up; ++l) ecc_change_level(Hm, false);
    double* st = state + (size_t)b * BH_ECC_STATE;
    for (int i = 0; i < 9; ++i) { st[ST_CUR + i] = Hm[i]; st[ST_BEST + i] = Hm[i]; }
    st[ST_RHO_BEST] = -__builtin_inf();
    for (int i = ST_FROZEN; i < BH_ECC_STATE; ++i) st[i] = 0.0;
}

// ------------------------------------------------------------------------------------------------
// the host side
// ------------------------------------------------------------------------------------------------
// what the entry points refuse as BH_E_BADARG apart from their NULL pointers: a negative batch or a plane without extent
static bool ecc_extents_bad(int count, int h, int w) { return count < 0 || h < 1 || w < 1; }

// BH_OK, or BH_E_UNSUPPORTED for a pyramid this file does not build: levels outside 1..6, a coarsest level under 8 pixels on a side, or
// more than 2^29 pixels (tap_place's offsets are ints of 4 bytes per pixel).  off[l] = the first float of level l, off[levels] = all of them.
static int ecc_layout(int H, int W, int levels, int64_t* off) {
    if (levels < 1 || levels > ECC_MAX_LEVELS || (H >> (levels - 1)) < ECC_MIN_SIDE || (W >> (levels - 1)) < ECC_MIN_SIDE) return BH_E_UNSUPPORTED;
    if ((long long)H * W > (1ll << 29)) return BH_E_UNSUPPORTED;
    int64_t at = 0;
    for (int l = 0; l < levels; ++l) {
        if (off) off[l] = at;
        at += (int64_t)(H >> l) * (W >> l);
    }
    if (off) off[levels] = at;
    return BH_OK;
}

static unsigned ecc_blocks(int Hb, int Wb) { return (unsigned)(((long long)Hb * Wb + ECC_BLOCK_PIXELS - 1) / ECC_BLOCK_PIXELS); }
static dim3 ecc_grid(unsigned x, int B) { return dim3(x, u8_grid_y(B)); }

static void ecc_launch_sums(const float* a, int Ha, int Wa, size_t a_stride, const float* t, int Hb, int Wb, size_t t_stride, const uint8_t* mask,
                            size_t m_stride, const double* H64, int h_stride, int B, double* partial, hipStream_t st) {
    if (mask)
        hipLaunchKernelGGL(ecc_sums_kernel<true>, ecc_grid(ecc_blocks(Hb, Wb), B), dim3(ECC_THREADS), 0, st, a, Ha, Wa, a_stride, t, Hb, Wb, t_stride,
                           mask, m_stride, H64, h_stride, B, partial);
    else
        hipLaunchKernelGGL(ecc_sums_kernel<false>, ecc_grid(ecc_blocks(Hb, Wb), B), dim3(ECC_THREADS), 0, st, a, Ha, Wa, a_stride, t, Hb, Wb, t_stride,
                           mask, m_stride, H64, h_stride, B, partial);
}

extern "C" {

int bh_gray_pyramid_layout(int H, int W, int levels, int64_t* offsets) {
    if (!offsets || H < 1 || W < 1) return BH_E_BADARG;
    return ecc_layout(H, W, levels, offsets);
}

int bh_gray_pyramid_u8(const uint8_t* images, const int* idx, int n_images, int H, int W, int B, int levels, float* pyr, void* stream) {
    if (!images || !pyr || ecc_extents_bad(B, H, W) || n_images < 1) return BH_E_BADARG;
    int64_t off[ECC_MAX_LEVELS + 1];
    const int rc = ecc_layout(H, W, levels, off);
    if (rc != BH_OK) return rc;
    if (B == 0) return BH_OK;
    hipStream_t st = bh_stream(stream);
    const size_t total = (size_t)off[levels];
    hipLaunchKernelGGL(ecc_gray_kernel, ecc_grid(((unsigned)(H * W) + ECC_THREADS - 1) / ECC_THREADS, B), dim3(ECC_THREADS), 0, st, images, idx, n_images,
                       H, W, B, total, pyr);
    for (int l = 1; l < levels; ++l) {
        const int hd = H >> l, wd = W >> l;
        hipLaunchKernelGGL(ecc_halve_kernel, ecc_grid(((unsigned)(hd * wd) + ECC_THREADS - 1) / ECC_THREADS, B), dim3(ECC_THREADS), 0, st, pyr, total,
                           (size_t)off[l - 1], W >> (l - 1), (size_t)off[l], hd, wd, B);
    }
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_ecc_sums_ws_doubles(int Hb, int Wb, int B, int64_t* doubles) {
    if (!doubles || ecc_extents_bad(B, Hb, Wb)) return BH_E_BADARG;
    if ((long long)Hb * Wb > (1ll << 29)) return BH_E_UNSUPPORTED;
    *doubles = (int64_t)B * ecc_blocks(Hb, Wb) * ECC_NS;
    return BH_OK;
}

int bh_ecc_sums(const float* a, int Ha, int Wa, int64_t a_stride, const float* t, int Hb, int Wb, int64_t t_stride, const uint8_t* mask,
                const double* H64, int B, double* partial, double* sums, void* stream) {
    if (!a || !t || !H64 || !partial || !sums || ecc_extents_bad(B, Ha, Wa) || Hb < 1 || Wb < 1) return BH_E_BADARG;
    if (a_stride < (int64_t)Ha * Wa || t_stride < (int64_t)Hb * Wb) return BH_E_BADARG;
    if ((long long)Ha * Wa > (1ll << 29) || (long long)Hb * Wb > (1ll << 29)) return BH_E_UNSUPPORTED;
    if (B == 0) return BH_OK;
    hipStream_t st = bh_stream(stream);
    ecc_launch_sums(a, Ha, Wa, (size_t)a_stride, t, Hb, Wb, (size_t)t_stride, mask, (size_t)Hb * Wb, H64, 9, B, partial, st);
    hipLaunchKernelGGL(ecc_reduce_kernel, dim3((unsigned)B), dim3(ECC_STEP_THREADS), 0, st, partial, (int)ecc_blocks(Hb, Wb), sums);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_ecc_step(const double* sums, double* state, int B, int last, double* stats, int stats_stride, void* stream) {
    if (!sums || !state || ecc_extents_bad(B, 1, 1) || last < 0 || last > 2 || (stats && stats_stride < 3)) return BH_E_BADARG;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(ecc_step_kernel<false>, dim3((unsigned)B), dim3(ECC_STEP_THREADS), 0, bh_stream(stream), sums, 0, state, last, stats,
                       stats_stride, (double*)nullptr);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_ecc_refine_ws_doubles(int Hb, int Wb, int B, int64_t* doubles) {
    if (!doubles || ecc_extents_bad(B, Hb, Wb)) return BH_E_BADARG;
    if ((long long)Hb * Wb > (1ll << 29)) return BH_E_UNSUPPORTED;
    *doubles = (int64_t)B * BH_ECC_STATE + (int64_t)B * ecc_blocks(Hb, Wb) * ECC_NS;
    return BH_OK;
}

int bh_ecc_refine(const float* pyr_a, int Ha, int Wa, const float* pyr_b, int Hb, int Wb, const uint8_t* mask_pyr, int B, int levels, int iters,
                  double* H64, double* stats, double* ws, void* stream) {
    if (!pyr_a || !pyr_b || !H64 || !stats || !ws || ecc_extents_bad(B, Ha, Wa) || Hb < 1 || Wb < 1 || iters < 0) return BH_E_BADARG;
    int64_t offa[ECC_MAX_LEVELS + 1], offb[ECC_MAX_LEVELS + 1];
    int rc = ecc_layout(Ha, Wa, levels, offa);
    if (rc == BH_OK) rc = ecc_layout(Hb, Wb, levels, offb);
    if (rc != BH_OK) return rc;
    if (B == 0) return BH_OK;
    hipStream_t st = bh_stream(stream);
    double* state = ws;
    double* partial = ws + (size_t)B * BH_ECC_STATE;
    hipLaunchKernelGGL(ecc_start_kernel, dim3((unsigned)(B + 63) / 64), dim3(64), 0, st, H64, B, levels - 1, state);
    for (int l = levels - 1; l >= 0; --l) {
        const int ha = Ha >> l, wa = Wa >> l, hb = Hb >> l, wb = Wb >> l;
        for (int k = 0; k <= iters; ++k) {
            ecc_launch_sums(pyr_a + offa[l], ha, wa, (size_t)offa[levels], pyr_b + offb[l], hb, wb, (size_t)offb[levels],
                            mask_pyr ? mask_pyr + offb[l] : nullptr, (size_t)offb[levels], state, BH_ECC_STATE, B, partial, st);
            const int last = k < iters ? 0 : (l > 0 ? 2 : 1);
            hipLaunchKernelGGL(ecc_step_kernel<true>, dim3((unsigned)B), dim3(ECC_STEP_THREADS), 0, st, partial, (int)ecc_blocks(hb, wb), state, last,
                               stats + 3 * l, 3 * levels, (last == 1) ? H64 : (double*)nullptr);
        }
    }
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
