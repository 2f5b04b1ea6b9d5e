// Global adjustment of a registered sequence (include/bihome.h "Global adjustment"; bihome_amd/align.py holds the numpy float64 statement
// adjust_host the kernel is tested against).  Upstream has nothing like it.
//
// bh_pano_adjust: Levenberg-Marquardt on all frames' homographies at once, one workgroup per sample, one launch, all double.  Per step:
//   form     the normal matrix edge by edge - 64 threads make the Jacobian rows of the edge's g x g points in LDS, 256 threads each sum one
//            entry of the four 8 x 8 blocks (a,a) (b,b) (a,b) (b,a) over the points and add it to the matrix in `ws`; the right-hand side
//            -J^T r is kept as row N of that matrix, so the factorisation does the forward substitution on the way
//   factor   blocked right-looking Cholesky, blocks of 8 (N = 8 (n - 1) has no partial block): the diagonal block in LDS by one thread,
//            the panel below it one row per thread into LDS, the trailing update one 8 x 8 tile per wavefront from that panel
//   solve    L^T d = y by blocks of 8 backwards, the right-hand side in LDS
//   trial    cost of W + d, one edge per thread, reduced through LDS in a fixed tree
// No atomics: every sum has one order, stated in the header.
#include "common.h"

#define ADJ_THREADS 256
#define ADJ_MAX_FRAMES 64
#define ADJ_MAX_EDGES 1024
#define ADJ_MAX_N (8 * (ADJ_MAX_FRAMES - 1))
#define ADJ_MAX_POINTS 64                      // grid 8
#define ADJ_REC 34                             // per point: Jx_a[8], Jy_a[8], Jx_b[8], Jy_b[8], rx, ry
#define ADJ_PANEL (8 * (ADJ_MAX_N - 8 + 1))    // the rows below the first diagonal block, row N (the right-hand side) among them

struct AdjShared {
    double big[ADJ_PANEL];                     // the Jacobian rows of one edge (ADJ_REC * points), or the Cholesky panel
    double W[9 * ADJ_MAX_FRAMES];
    double Wt[9 * ADJ_MAX_FRAMES];
    double rhs[ADJ_MAX_N];
    double red[ADJ_THREADS];
    double Lkk[64];
    double cost, cost_t, lambda;
    int touched[ADJ_MAX_FRAMES];
    int flag, failed, accepted;
};

// the lattice point p = j g + i of the frame
__device__ __forceinline__ void adj_point(int p, int g, int Hs, int Ws, double& x, double& y) {
    x = (double)((p % g) * (Ws - 1)) / (double)(g - 1);
    y = (double)((p / g) * (Hs - 1)) / (double)(g - 1);
}

// q = M (x, y, 1) with M used as it is; -> qz, (u, v) = (qx, qy) / qz
__device__ __forceinline__ double adj_project(const double* M, double x, double y, double& u, double& v) {
#pragma clang fp contract(off)
    const double qx = (M[0] * x + M[1] * y) + M[2], qy = (M[3] * x + M[4] * y) + M[5], qz = (M[6] * x + M[7] * y) + M[8];
    u = qx / qz;
    v = qy / qz;
    return qz;
}

// H / H[8] of a link
__device__ __forceinline__ void adj_link(const double* H, double* h) {
    const double s = H[8];
    for (int i = 0; i < 9; ++i) h[i] = H[i] / s;
}

__device__ __forceinline__ bool adj_edge_counts(const int* link, const double* weight, int e, int n, int& a, int& b, double& w) {
    a = link[2 * e];
    b = link[2 * e + 1];
    w = weight ? weight[e] : 1.0;
    return a != b && a >= 0 && a < n && b >= 0 && b < n && isfinite(w) && w > 0.0;
}

// adjugate of a 3 x 3 and its determinant by the adjugate's first column, (a adj00 + b adj10) + c adj20
__device__ __forceinline__ double adj_adjugate(const double* g, double* adj) {
#pragma clang fp contract(off)
    const double a = g[0], b = g[1], c = g[2], d = g[3], e = g[4], f = g[5], gg = g[6], h = g[7], i = g[8];
    adj[0] = e * i - f * h; adj[1] = c * h - b * i; adj[2] = b * f - c * e;
    adj[3] = f * gg - d * i; adj[4] = a * i - c * gg; adj[5] = c * d - a * f;
    adj[6] = d * h - e * gg; adj[7] = b * gg - a * h; adj[8] = a * e - b * d;
    return (a * adj[0] + b * adj[3]) + c * adj[6];
}

// cost of the matrices Wm (LDS) -> s.red[0] after the tree; s.flag cleared where a counting point has qz <= 0 (or NaN) under the link or
// under either matrix.  Every thread returns the same cost.
__device__ double adj_cost(AdjShared& s, const double* Wm, const int* link, const double* Hl, const double* weight, int n, int E, int g, int Hs, int Ws) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double part = 0.0;
    bool ok = true;
    for (int e = tid; e < E; e += ADJ_THREADS) {
        int a, b;
        double w;
        if (!adj_edge_counts(link, weight, e, n, a, b, w)) continue;
        double h[9];
        adj_link(Hl + 9 * e, h);
        double se = 0.0;
        for (int p = 0; p < g * g; ++p) {
            double x, y, zx, zy, ua, va, ub, vb;
            adj_point(p, g, Hs, Ws, x, y);
            const double qh = adj_project(h, x, y, zx, zy);
            const double qa = adj_project(Wm + 9 * a, zx, zy, ua, va);
            const double qb = adj_project(Wm + 9 * b, x, y, ub, vb);
            ok = ok && qh > 0.0 && qa > 0.0 && qb > 0.0;
            const double rx = ua - ub, ry = va - vb;
            se += rx * rx + ry * ry;
        }
        part += w * se;
    }
    __syncthreads();                                                           // (red and flag may still be read from the call before)
    s.red[tid] = part;
    if (tid == 0) s.flag = 1;
    __syncthreads();
    if (!ok) s.flag = 0;
    for (int half = ADJ_THREADS / 2; half > 0; half >>= 1) {
        __syncthreads();
        if (tid < half) s.red[tid] += s.red[tid + half];
    }
    __syncthreads();
    return s.red[0];
}

// grid B, ADJ_THREADS threads
__global__ void __launch_bounds__(ADJ_THREADS) pano_adjust_kernel(const double* __restrict__ G0, const int* __restrict__ link, const double* __restrict__ Hlink,
                                                                  const double* __restrict__ weight, int n, int E, int ref, int Hs, int Ws, int g, int iters,
                                                                  double* __restrict__ G, double* __restrict__ work, double* __restrict__ ws) {
    __shared__ AdjShared s;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int N = 8 * (n - 1), P = g * g;
    const double* G0b = G0 + 9 * b * n;
    const double* Hl = Hlink + 9 * b * E;
    const double* wt = weight ? weight + b * E : nullptr;
    double* Gb = G + 9 * b * n;
    double* M = ws + b * ((size_t)N + 1) * N;                                  // [N + 1, N] row-major; row N is the right-hand side

    // ---- the start: finite inputs, W = adj(G0) / adj[2,2], which frames an edge touches -------------------------------------------------
    if (tid == 0) { s.flag = 1; s.failed = 0; s.accepted = 0; s.lambda = 1e-3; }
    if (tid < n) s.touched[tid] = 0;
    __syncthreads();
    bool fine = true;
    for (int i = tid; i < 9 * n; i += ADJ_THREADS) fine = fine && isfinite(G0b[i]);
    for (int e = tid; e < E; e += ADJ_THREADS) {
        int fa, fb;
        double w;
        if (!adj_edge_counts(link, wt, e, n, fa, fb, w)) continue;
        for (int i = 0; i < 9; ++i) fine = fine && isfinite(Hl[9 * e + i]);
        s.touched[fa] = 1;                                                     // (every writer stores the same value)
        s.touched[fb] = 1;
    }
    if (tid < n) {
        double adj[9];
        const double det = adj_adjugate(G0b + 9 * tid, adj);
        const bool isref = tid == ref;
        if (!isref) fine = fine && isfinite(det) && det != 0.0;
        for (int i = 0; i < 9; ++i) {
            const double v = isref ? (i % 4 == 0 ? 1.0 : 0.0) : adj[i] / adj[8];
            fine = fine && isfinite(v);
            s.W[9 * tid + i] = v;
        }
    }
    if (!fine) s.flag = 0;
    __syncthreads();
    const bool inputs_ok = s.flag != 0;
    __syncthreads();
    double cost0 = __longlong_as_double(0x7ff8000000000000ll);                 // NaN: the start could not be evaluated
    bool start_ok = false;
    if (inputs_ok) {
        cost0 = adj_cost(s, s.W, link, Hl, wt, n, E, g, Hs, Ws);
        start_ok = s.flag != 0 && isfinite(cost0);
    }
    if (tid == 0) s.cost = cost0;
    __syncthreads();

    if (start_ok) {
        for (int it = 0; it < iters; ++it) {
            const double lambda = s.lambda;
            // ---- form: zero, then edge by edge ------------------------------------------------------------------------------------------
            for (size_t i = tid; i < ((size_t)N + 1) * N; i += ADJ_THREADS) M[i] = 0.0;
            __syncthreads();
            for (int e = 0; e < E; ++e) {
                int fa, fb;
                double w;
                if (!adj_edge_counts(link, wt, e, n, fa, fb, w)) continue;     // (the same for every thread)
                if (tid < P) {
#pragma clang fp contract(off)
                    double h[9], x, y, zx, zy, ua, va, ub, vb;
                    adj_link(Hl + 9 * e, h);
                    adj_point(tid, g, Hs, Ws, x, y);
                    adj_project(h, x, y, zx, zy);
                    const double qa = adj_project(s.W + 9 * fa, zx, zy, ua, va);
                    const double qb = adj_project(s.W + 9 * fb, x, y, ub, vb);
                    double* r = s.big + ADJ_REC * tid;
                    const double ax = zx / qa, ay = zy / qa, a1 = 1.0 / qa, bx = x / qb, by = y / qb, b1 = 1.0 / qb;
                    r[0] = ax; r[1] = ay; r[2] = a1; r[3] = 0.0; r[4] = 0.0; r[5] = 0.0; r[6] = -(ax * ua); r[7] = -(ay * ua);
                    r[8] = 0.0; r[9] = 0.0; r[10] = 0.0; r[11] = ax; r[12] = ay; r[13] = a1; r[14] = -(ax * va); r[15] = -(ay * va);
                    r[16] = -bx; r[17] = -by; r[18] = -b1; r[19] = 0.0; r[20] = 0.0; r[21] = 0.0; r[22] = bx * ub; r[23] = by * ub;
                    r[24] = 0.0; r[25] = 0.0; r[26] = 0.0; r[27] = -bx; r[28] = -by; r[29] = -b1; r[30] = bx * vb; r[31] = by * vb;
                    r[32] = ua - ub; r[33] = va - vb;
                }
                __syncthreads();
                {
#pragma clang fp contract(off)
                    const int q = tid >> 6, rr = (tid >> 3) & 7, cc = tid & 7;
                    const int fr = (q == 0 || q == 2) ? fa : fb, fc = (q == 0 || q == 3) ? fa : fb;      // the frames of the block's rows and columns
                    const int orow = (fr == fa ? 0 : 16) + rr, ocol = (fc == fa ? 0 : 16) + cc;
                    if (fr != ref && fc != ref) {
                        const int row = 8 * (fr < ref ? fr : fr - 1) + rr, col = 8 * (fc < ref ? fc : fc - 1) + cc;
                        if (row >= col) {                                      // the lower triangle is all the factorisation reads
                            double acc = 0.0;
                            for (int p = 0; p < P; ++p) {
                                const double* r = s.big + ADJ_REC * p;
                                acc += r[orow] * r[ocol] + r[orow + 8] * r[ocol + 8];
                            }
                            M[(size_t)row * N + col] += w * acc;
                        }
                        if (q < 2 && cc == 0) {                                // -J^T r, the frame's eight entries
                            double acc = 0.0;
                            for (int p = 0; p < P; ++p) {
                                const double* r = s.big + ADJ_REC * p;
                                acc += r[orow] * r[32] + r[orow + 8] * r[33];
                            }
                            M[(size_t)N * N + row] -= w * acc;
                        }
                    }
                }
                __syncthreads();
            }
            // ---- the damping; unit rows for the frames no edge touches ------------------------------------------------------------------
            for (int i = tid; i < N; i += ADJ_THREADS) {
#pragma clang fp contract(off)
                const int slot = i >> 3, frame = slot < ref ? slot : slot + 1;
                const double d = M[(size_t)i * N + i];
                M[(size_t)i * N + i] = s.touched[frame] ? d + lambda * d : 1.0;
            }
            __syncthreads();
            // ---- factor -----------------------------------------------------------------------------------------------------------------
            for (int k0 = 0; k0 < N; k0 += 8) {
                if (tid < 64) {
                    const int rr = tid >> 3, cc = tid & 7;
                    s.Lkk[tid] = cc <= rr ? M[(size_t)(k0 + rr) * N + k0 + cc] : 0.0;
                }
                __syncthreads();
                if (tid == 0) {
                    for (int j = 0; j < 8; ++j) {
                        double d = s.Lkk[8 * j + j];
                        for (int c = 0; c < j; ++c) d = fma(-s.Lkk[8 * j + c], s.Lkk[8 * j + c], d);
                        if (!(d > 0.0)) s.failed = 1;                          // (NaN too)
                        d = sqrt(d);
                        s.Lkk[8 * j + j] = d;
                        for (int i = j + 1; i < 8; ++i) {
                            double v = s.Lkk[8 * i + j];
                            for (int c = 0; c < j; ++c) v = fma(-s.Lkk[8 * i + c], s.Lkk[8 * j + c], v);
                            s.Lkk[8 * i + j] = v / d;
                        }
                    }
                }
                __syncthreads();
                if (s.failed) break;
                if (tid < 64 && (tid & 7) <= (tid >> 3)) M[(size_t)(k0 + (tid >> 3)) * N + k0 + (tid & 7)] = s.Lkk[tid];
                const int below = N + 1 - (k0 + 8);                            // rows under the block, the right-hand side the last of them
                for (int i = tid; i < below; i += ADJ_THREADS) {
                    double* row = M + (size_t)(k0 + 8 + i) * N + k0;
                    double x[8];
                    for (int j = 0; j < 8; ++j) {
                        double v = row[j];
                        for (int c = 0; c < j; ++c) v = fma(-x[c], s.Lkk[8 * j + c], v);
                        x[j] = v / s.Lkk[8 * j + j];
                    }
                    for (int j = 0; j < 8; ++j) { row[j] = x[j]; s.big[8 * i + j] = x[j]; }
                }
                __syncthreads();
                const int T = (N - (k0 + 8)) / 8;                              // trailing tiles per side
                for (int tile = tid >> 6; tile < T * T; tile += ADJ_THREADS / 64) {
                    const int bi = tile / T, bj = tile - bi * T;
                    if (bj > bi) continue;
                    const int rr = (tid >> 3) & 7, cc = tid & 7;
                    if (bi == bj && cc > rr) continue;
                    const double* pi = s.big + 8 * (8 * bi + rr);
                    const double* pj = s.big + 8 * (8 * bj + cc);
                    double* at = M + (size_t)(k0 + 8 + 8 * bi + rr) * N + (k0 + 8 + 8 * bj + cc);
                    double v = *at;
                    for (int c = 0; c < 8; ++c) v = fma(-pi[c], pj[c], v);
                    *at = v;
                }
                for (int j = tid; j < 8 * T; j += ADJ_THREADS) {               // the right-hand side's row
                    const double* pi = s.big + 8 * (8 * T);
                    const double* pj = s.big + 8 * j;
                    double* at = M + (size_t)N * N + (k0 + 8 + j);
                    double v = *at;
                    for (int c = 0; c < 8; ++c) v = fma(-pi[c], pj[c], v);
                    *at = v;
                }
                __syncthreads();
            }
            if (s.failed) break;
            // ---- solve L^T d = y ----------------------------------------------------------------------------------------------------------
            for (int i = tid; i < N; i += ADJ_THREADS) s.rhs[i] = M[(size_t)N * N + i];
            __syncthreads();
            for (int k0 = N - 8; k0 >= 0; k0 -= 8) {
                if (tid < 64) s.Lkk[tid] = M[(size_t)(k0 + (tid >> 3)) * N + k0 + (tid & 7)];        // (the lower half is what is read)
                __syncthreads();
                if (tid == 0) {
                    for (int j = 7; j >= 0; --j) {
                        double v = s.rhs[k0 + j];
                        for (int c = 7; c > j; --c) v = fma(-s.Lkk[8 * c + j], s.rhs[k0 + c], v);
                        s.rhs[k0 + j] = v / s.Lkk[8 * j + j];
                    }
                }
                __syncthreads();
                for (int j = tid; j < k0; j += ADJ_THREADS) {
                    double v = s.rhs[j];
                    for (int c = 0; c < 8; ++c) v = fma(-M[(size_t)(k0 + c) * N + j], s.rhs[k0 + c], v);
                    s.rhs[j] = v;
                }
                __syncthreads();
            }
            // ---- the trial --------------------------------------------------------------------------------------------------------------
            bool finite = true;
            for (int i = tid; i < N; i += ADJ_THREADS) finite = finite && isfinite(s.rhs[i]);
            if (!finite) s.failed = 1;
            for (int i = tid; i < 9 * n; i += ADJ_THREADS) {
                const int k = i / 9, c = i - 9 * k;
                s.Wt[i] = (k == ref || c == 8) ? s.W[i] : s.W[i] + s.rhs[8 * (k < ref ? k : k - 1) + c];
            }
            __syncthreads();
            if (s.failed) break;
            const double ct = adj_cost(s, s.Wt, link, Hl, wt, n, E, g, Hs, Ws);
            const bool accept = isfinite(ct) && s.flag != 0 && ct < s.cost;
            __syncthreads();
            if (accept)
                for (int i = tid; i < 9 * n; i += ADJ_THREADS) s.W[i] = s.Wt[i];
            if (tid == 0) {
                if (accept) { s.cost = ct; s.accepted += 1; s.lambda = fmax(lambda / 10.0, 1e-12); }
                else s.lambda = fmin(lambda * 10.0, 1e12);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- the result: G = adj(W) / adj[2,2], or the start ----------------------------------------------------------------------------------
    bool moved = start_ok && !s.failed && s.accepted > 0;
    if (tid == 0) s.flag = 1;
    __syncthreads();
    if (moved && tid < n) {
        double adj[9];
        adj_adjugate(s.W + 9 * tid, adj);
        bool finite = true;
        for (int i = 0; i < 9; ++i) {
            const double v = tid == ref ? (i % 4 == 0 ? 1.0 : 0.0) : adj[i] / adj[8];
            finite = finite && isfinite(v);
            s.Wt[9 * tid + i] = v;
        }
        if (!finite) s.flag = 0;
    }
    __syncthreads();
    moved = moved && s.flag != 0;
    for (int i = tid; i < 9 * n; i += ADJ_THREADS) Gb[i] = moved ? s.Wt[i] : G0b[i];
    if (tid == 0) {
        work[4 * b] = cost0;
        work[4 * b + 1] = moved ? s.cost : cost0;
        work[4 * b + 2] = moved ? (double)s.accepted : 0.0;
        work[4 * b + 3] = s.lambda;
    }
}

// what the entry points refuse as BH_E_BADARG apart from their NULL pointers
static bool adjust_counts_bad(int count, int frames, int edges) {
    return count < 0 || frames < 2 || frames > ADJ_MAX_FRAMES || edges < 1 || edges > ADJ_MAX_EDGES;
}

extern "C" {

int bh_pano_adjust_ws_doubles(int n, int E, int B, int64_t* doubles) {
    if (!doubles || adjust_counts_bad(B, n, E)) return BH_E_BADARG;
    const int64_t N = 8 * ((int64_t)n - 1);
    *doubles = (int64_t)B * (N + 1) * N;
    return BH_OK;
}

int bh_pano_adjust(const double* G0, const int* link, const double* Hlink, const double* weight, int B, int n, int E, int ref, int Hs, int Ws,
                   int grid, int iters, double* G, double* work, double* ws, void* stream) {
    if (!G0 || !link || !Hlink || !G || !work || !ws || adjust_counts_bad(B, n, E) || ref < 0 || ref >= n || Hs < 2 || Ws < 2 || Hs > (1 << 24) ||
        Ws > (1 << 24) || grid < 2 || grid > 8 || iters < 0)
        return BH_E_BADARG;
    if (B == 0) return BH_OK;
    hipLaunchKernelGGL(pano_adjust_kernel, dim3((unsigned)B), dim3(ADJ_THREADS), 0, bh_stream(stream), G0, link, Hlink, weight, n, E, ref, Hs, Ws, grid, iters, G,
                       work, ws);
    BH_LAUNCH_CHECK();
    return BH_OK;
}

}  // extern "C"
