// Panorama, the geometry: the chain and the canvas of a registered sequence (include/bihome.h "Panorama"; bihome_amd/align.py holds the
// numpy float64 statements chain_host / pano_frame_host the kernels are tested against).  Upstream has nothing like it.  The blend of
// the frames on that canvas, bh_pano_u8, is csrc/blend.hip's.
//
// bh_pano_chain: the n - 1 pair homographies of a sequence composed into G[k], the reference's index coordinates -> frame k's, outwards
// from the reference; one thread per sample, double.
// bh_pano_frame: the canvas around the reference's extent and every frame's projected corners - adjugate, corners, the usable test and
// the clamp per frame (thread k), a min / max reduction over the workgroup, then T, the box and M[k] = G[k] T; one workgroup per sample,
// one launch.  The reference has a size of its own, so the pair's frame (align.py mosaic_frame_device) is this kernel with n = 1.
#include "common.h"

#define PANO_THREADS 256
#define PANO_MAX_FRAMES 255

// ------------------------------------------------------------------------------------------------
// the chain
// ------------------------------------------------------------------------------------------------
// grid ceil(B / PANO_THREADS)
__global__ void __launch_bounds__(PANO_THREADS) pano_chain_kernel(const double* __restrict__ Hpair, const double* __restrict__ gain_pair, int B, int n, int ref,
                                                                  double* __restrict__ G, double* __restrict__ gain) {
#pragma clang fp contract(off)
    const size_t b = (size_t)blockIdx.x * PANO_THREADS + threadIdx.x;
    if (b >= (size_t)B) return;
    double* Gb = G + 9 * b * n;
    const double* Hb = Hpair + 9 * b * (n - 1);
    const bool lines = gain && (gain_pair || n == 1);                           // (a single frame has no pair: its line is (1, 0))
    double* gb = lines ? gain + 2 * b * n : nullptr;
    const double* pb = lines ? gain_pair + 2 * b * (n - 1) : nullptr;
    for (int i = 0; i < 9; ++i) Gb[9 * ref + i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (lines) { gb[2 * ref] = 1.0; gb[2 * ref + 1] = 0.0; }
    for (int step = 0; step < n - 1; ++step) {
        const int j = step < n - 1 - ref ? ref + step : n - 2 - step;          // ref .. n - 2, then ref - 1 .. 0
        const int fa = j >= ref ? j + 1 : j, fb = j >= ref ? j : j + 1;         // the pair (a, b): b is nearer to the reference and done
        const double* H = Hb + 9 * j;
        double L[9], P[9];
        for (int i = 0; i < 9; ++i) L[i] = Gb[9 * fb + i];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) P[3 * r + c] = (H[3 * r] * L[c] + H[3 * r + 1] * L[3 + c]) + H[3 * r + 2] * L[6 + c];
        for (int i = 0; i < 9; ++i) Gb[9 * fa + i] = P[i] / P[8];
        if (lines) {
            const double g_b = gb[2 * fb], o_b = gb[2 * fb + 1];
            gb[2 * fa] = g_b * pb[2 * j];
            gb[2 * fa + 1] = g_b * pb[2 * j + 1] + o_b;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the frame
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pano_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double pano_clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// grid B, PANO_THREADS threads: thread k is frame k (n <= PANO_MAX_FRAMES).  Hs x Ws: the frames, whose corners are projected; Hr x Wr: the
// reference, whose extent starts the box and scales the clamp
__global__ void __launch_bounds__(PANO_THREADS) pano_frame_kernel(const double* __restrict__ G, const unsigned char* __restrict__ use, int n, int Hs, int Ws,
                                                                  int Hr, int Wr, int Hc, int Wc, double limit, double* __restrict__ T,
                                                                  double* __restrict__ bbox, unsigned char* __restrict__ fitted, double* __restrict__ M) {
#pragma clang fp contract(off)
    __shared__ double red[4][PANO_THREADS / 64];
    __shared__ double Ts[3];                                                   // s, tx, ty
    const size_t b = blockIdx.x;
    const int k = threadIdx.x;
    const double W1 = (double)Ws - 1.0, H1 = (double)Hs - 1.0, Wr1 = (double)Wr - 1.0, Hr1 = (double)Hr - 1.0;
    double x0 = 0.0, x1 = Wr1, y0 = 0.0, y1 = Hr1, g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (k < n) {
        const double* Gk = G + 9 * (b * n + k);
        for (int i = 0; i < 9; ++i) g[i] = Gk[i];
        const double a = g[0], bb = g[1], c = g[2], d = g[3], e = g[4], f = g[5], gg = g[6], h = g[7], i = g[8];
        const double adj[9] = {e * i - f * h, c * h - bb * i, bb * f - c * e, f * gg - d * i, a * i - c * gg, c * d - a * f, d * h - e * gg, bb * gg - a * h, a * e - bb * d};
        const double det = (a * adj[0] + bb * adj[3]) + c * adj[6];
        double inv[9];
        for (int q = 0; q < 9; ++q) inv[q] = adj[q] / det;
        const double cx[4] = {0.0, W1, W1, 0.0}, cy[4] = {0.0, 0.0, H1, H1};
        bool usable = isfinite(det) && det != 0.0, pos = true, neg = true;
        double pxmin = 0, pxmax = 0, pymin = 0, pymax = 0;
        for (int q = 0; q < 4; ++q) {
            const double qx = (inv[0] * cx[q] + inv[1] * cy[q]) + inv[2], qy = (inv[3] * cx[q] + inv[4] * cy[q]) + inv[5], qz = (inv[6] * cx[q] + inv[7] * cy[q]) + inv[8];
            const double px = qx / qz, py = qy / qz;
            usable = usable && isfinite(qz) && fabs(qz) > 1e-8 && isfinite(px) && isfinite(py);
            pos = pos && qz > 0.0;
            neg = neg && qz < 0.0;
            pxmin = q ? fmin(pxmin, px) : px; pxmax = q ? fmax(pxmax, px) : px;
            pymin = q ? fmin(pymin, py) : py; pymax = q ? fmax(pymax, py) : py;
        }
        usable = usable && (pos || neg) && !(use && use[b * n + k] == 0);
        if (usable) {
            const double W = (double)Wr, H = (double)Hr;
            x0 = fmin(pano_clip(pxmin, -limit * W, (1.0 + limit) * W - 1.0), 0.0);
            x1 = fmax(pano_clip(pxmax, -limit * W, (1.0 + limit) * W - 1.0), Wr1);
            y0 = fmin(pano_clip(pymin, -limit * H, (1.0 + limit) * H - 1.0), 0.0);
            y1 = fmax(pano_clip(pymax, -limit * H, (1.0 + limit) * H - 1.0), Hr1);
        }
        if (fitted) fitted[b * n + k] = usable ? 1 : 0;
    }
    // min / max are exact: the order of the reduction does not show
    x0 = pano_wave_min(x0); x1 = -pano_wave_min(-x1); y0 = pano_wave_min(y0); y1 = -pano_wave_min(-y1);
    if ((k & 63) == 0) { red[0][k >> 6] = x0; red[1][k >> 6] = x1; red[2][k >> 6] = y0; red[3][k >> 6] = y1; }
    __syncthreads();
    if (k == 0) {
        for (int w = 1; w < PANO_THREADS / 64; ++w) { x0 = fmin(x0, red[0][w]); x1 = fmax(x1, red[1][w]); y0 = fmin(y0, red[2][w]); y1 = fmax(y1, red[3][w]); }
        double s = fmax((x1 - x0) / (double)(Wc - 1), (y1 - y0) / (double)(Hc - 1));
        s = s == 0.0 ? 1.0 : s;
        const double tx = (x0 + x1) * 0.5 - s * (0.5 * (double)(Wc - 1)), ty = (y0 + y1) * 0.5 - s * (0.5 * (double)(Hc - 1));
        Ts[0] = s; Ts[1] = tx; Ts[2] = ty;
        double* Tb = T + 9 * b;
        Tb[0] = s; Tb[1] = 0.0; Tb[2] = tx; Tb[3] = 0.0; Tb[4] = s; Tb[5] = ty; Tb[6] = 0.0; Tb[7] = 0.0; Tb[8] = 1.0;
        if (bbox) { bbox[4 * b] = x0; bbox[4 * b + 1] = y0; bbox[4 * b + 2] = x1; bbox[4 * b + 3] = y1; }
    }
    __syncthreads();
    if (M && k < n) {                                                          // G T with T = (s 0 tx; 0 s ty; 0 0 1)
        const double s = Ts[0], tx = Ts[1], ty = Ts[2];
        double* Mk = M + 9 * (b * n + k);
        for (int r = 0; r < 3; ++r) {
            Mk[3 * r] = g[3 * r] * s;
            Mk[3 * r + 1] = g[3 * r + 1] * s;
            Mk[3 * r + 2] = (g[3 * r] * tx + g[3 * r + 1] * ty) + g[3 * r + 2];
        }
    }
}

// what the entry points refuse as BH_E_BADARG apart from their NULL pointers: a negative batch, a frame count outside 1..255, an extent
// below `least`
static bool pano_counts_bad(int count, int frames) { return count < 0 || frames < 1 || frames > PANO_MAX_FRAMES; }
static bool pano_extents_bad(int Hs, int Ws, int Hc, int Wc, int least) { return Hs < 1 || Ws < 1 || Hc < least || Wc < least; }

extern "C" {

int bh_pano_chain(const double* Hpair, const double* gain_pair, int B, int n, int ref, double* G, double* gain, void* stream) {
    if (!G || pano_counts_bad(B, n) || (!Hpair && n > 1) || ref < 0 || ref >= n) return BH_E_BADARG;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(pano_chain_kernel, dim3(((unsigned)B + PANO_THREADS - 1) / PANO_THREADS), dim3(PANO_THREADS), 0, bh_stream(stream), Hpair, gain_pair, B, n,
                       ref, G, gain);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

int bh_pano_frame(const double* G, const uint8_t* use, int B, int n, int Hs, int Ws, int Hr, int Wr, int Hc, int Wc, double limit,
                  double* T, double* bbox, uint8_t* fitted, double* M, void* stream) {
    if (!G || !T || pano_counts_bad(B, n) || pano_extents_bad(Hs, Ws, Hc, Wc, 2) || Hr < 1 || Wr < 1 || !(limit > 0.0)) return BH_E_BADARG;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(pano_frame_kernel, dim3((unsigned)B), dim3(PANO_THREADS), 0, bh_stream(stream), G, use, n, Hs, Ws, Hr, Wr, Hc, Wc, limit, T, bbox,
                       fitted, M);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
