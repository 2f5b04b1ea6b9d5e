// Device helpers of the per-sample dense algebra shared by csrc/geometry.hip (4-point solve, sampled DLT) and csrc/ransac.hip
// (minimal-sample hypotheses, inlier refit): the 8x8 solve, the 9x9 Jacobi eigen-solve and the DLT's normal matrix / epilogue.
// All arithmetic in double.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------
// 8x8 solve with partial pivoting; S is an 8x9 augmented system in LDS, row stride 9.
// On return the diagonal of S holds the eight pivots (a zero or NaN one: the system is singular and x holds inf / NaN).
// ---------------------------------------------------------------------------------------------
__device__ static void solve8(double* S, double* x) {
    for (int k = 0; k < 8; ++k) {
        int r = k;
        double best = fabs(S[k * 9 + k]);
        for (int i = k + 1; i < 8; ++i) {
            double v = fabs(S[i * 9 + k]);
            if (v > best) { best = v; r = i; }
        }
        if (r != k)
            for (int j = k; j < 9; ++j) { double t = S[k * 9 + j]; S[k * 9 + j] = S[r * 9 + j]; S[r * 9 + j] = t; }
        double inv = 1.0 / S[k * 9 + k];
        for (int i = k + 1; i < 8; ++i) {
            double f = S[i * 9 + k] * inv;
            for (int j = k + 1; j < 9; ++j) S[i * 9 + j] -= f * S[k * 9 + j];
        }
    }
    for (int k = 7; k >= 0; --k) {
        double acc = S[k * 9 + 8];
        for (int j = k + 1; j < 8; ++j) acc -= S[k * 9 + j] * x[j];
        x[k] = acc / S[k * 9 + k];
    }
}

__device__ static void corner_xy(int i, double W, double H, double& x, double& y) {
    // image_shape_to_corners: [[0,0],[W,0],[W,H],[0,H]]
    x = (i == 1 || i == 2) ? W : 0.0;
    y = (i >= 2) ? H : 0.0;
}

struct Hartley {
    double mx, my, s, dbar;
};

// Jacobi eigen-decomposition of the symmetric 9x9 matrix in LDS A (destroyed); V gets eigenvectors in columns.
// Parallel (round-robin) ordering: round r of a sweep rotates the four disjoint pairs {(r+k) mod 9, (r-k) mod 9},
// k = 1..4 (index r sits out; every pair {a, b} occurs once per sweep, in the round with 2r = a+b mod 9), so a sweep is
// 9 dependent steps instead of 36.  The rotations of a round commute (disjoint index pairs): first A J and V J
// (lane = (row, pair), columns p and q), then J^T (A J) (lane = (column, pair), rows p and q).
// One wave per workgroup (the barriers are workgroup barriers and the convergence test a wave sum).
__device__ static void jacobi9(double* A, double* V, int lane) {
    if (lane < 9)
        for (int j = 0; j < 9; ++j) V[lane * 9 + j] = (lane == j) ? 1.0 : 0.0;
    __syncthreads();
    const int k = lane >> 2, pr = lane & 3;       // lanes 0..35: row / column k, pair pr
    for (int sweep = 0; sweep < 16; ++sweep) {
        // convergence: off-diagonal mass vs diagonal mass
        double off = 0, dia = 0;
        if (lane < 9)
            for (int j = 0; j < 9; ++j) { double v = A[lane * 9 + j]; if (j == lane) dia += v * v; else off += v * v; }
        off = wave_sum(off); dia = wave_sum(dia);
        if (off <= 1e-30 * dia || off == 0.0) break;      // off-diagonal Frobenius mass below 1e-15 of the diagonal: converged in double
        for (int r = 0; r < 9; ++r) {
            int ia = r + pr + 1, ib = r + 8 - pr;
            ia = ia >= 9 ? ia - 9 : ia; ib = ib >= 9 ? ib - 9 : ib;
            const int p = min(ia, ib), q = max(ia, ib);
            const double apq = A[p * 9 + q], app = A[p * 9 + p], aqq = A[q * 9 + q];
            double c = 1.0, s = 0.0;
            if (fabs(apq) > 1e-300) {
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                c = 1.0 / sqrt(t * t + 1.0); s = t * c;
            }
            __syncthreads();                      // every lane has read its pair's entries
            if (k < 9) {
                const double akp = A[k * 9 + p], akq = A[k * 9 + q];
                A[k * 9 + p] = c * akp - s * akq;
                A[k * 9 + q] = s * akp + c * akq;
                const double vkp = V[k * 9 + p], vkq = V[k * 9 + q];
                V[k * 9 + p] = c * vkp - s * vkq;
                V[k * 9 + q] = s * vkp + c * vkq;
            }
            __syncthreads();
            if (k < 9) {
                const double apk = A[p * 9 + k], aqk = A[q * 9 + k];
                A[p * 9 + k] = c * apk - s * aqk;
                A[q * 9 + k] = s * apk + c * aqk;
            }
            __syncthreads();
        }
    }
    __syncthreads();
}

// The 24 sums a DLT keeps per point set - S0 = a a^T, Sx = x2 a a^T, Sy = y2 a a^T, Sr = (x2^2 + y2^2) a a^T with a = [x1 y1 1], all
// Hartley-normalised, six uniques each - added for one correspondence
__device__ __forceinline__ void dlt_accumulate(double* acc, const Hartley& t1, const Hartley& t2, double x1, double y1, double x2,
                                               double y2) {
    double a0 = t1.s * (x1 - t1.mx), a1 = t1.s * (y1 - t1.my), a2 = 1.0;
    double u = t2.s * (x2 - t2.mx), v = t2.s * (y2 - t2.my);
    double aa[6] = {a0 * a0, a0 * a1, a0 * a2, a1 * a1, a1 * a2, a2 * a2};
    double r = u * u + v * v;
    for (int i = 0; i < 6; ++i) {
        acc[i] += aa[i]; acc[6 + i] += u * aa[i]; acc[12 + i] += v * aa[i]; acc[18 + i] += r * aa[i];
    }
}

// ... and the 9x9 normal matrix A^T A (LDS, 81 doubles) they make; one lane
__device__ __forceinline__ void dlt_normal_matrix(double* A, const double* acc) {
    // symmetric 3x3 from 6 uniques: index map
    const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            int s = sym[r][c];
            A[(r) * 9 + c] = acc[s];                 // M00  (ay: [a,0,-x2 a])
            A[(3 + r) * 9 + 3 + c] = acc[s];         // M11  (ax: [0,-a,y2 a])
            A[(r) * 9 + 3 + c] = 0; A[(3 + r) * 9 + c] = 0;
            A[(r) * 9 + 6 + c] = -acc[6 + s]; A[(6 + r) * 9 + c] = -acc[6 + s];         // M02 = -Sx
            A[(3 + r) * 9 + 6 + c] = -acc[12 + s]; A[(6 + r) * 9 + 3 + c] = -acc[12 + s]; // M12 = -Sy
            A[(6 + r) * 9 + 6 + c] = acc[18 + s];    // M22 = Sr
        }
}

// The DLT's epilogue after jacobi9(A, V): eigenvector m of the smallest eigenvalue, denormalise, /(H22 + 1e-8) -> Hout[9] (fp32) and
// delta_hat[4,2] = H.corners - corners with corners [[0,0],[w,0],[w,h],[0,h]]; one lane.  Returns m.
__device__ __forceinline__ int dlt_epilogue(const double* A, const double* V, const Hartley& t1, const Hartley& t2, int w, int h,
                                            float* __restrict__ Hout, float* __restrict__ delta_hat) {
    int m = 0;
    for (int i = 1; i < 9; ++i) if (A[i * 9 + i] < A[m * 9 + m]) m = i;
    double Hh[9];
    for (int i = 0; i < 9; ++i) Hh[i] = V[i * 9 + m];
    double T1[9] = {t1.s, 0, -t1.s * t1.mx, 0, t1.s, -t1.s * t1.my, 0, 0, 1};
    double T2i[9] = {1.0 / t2.s, 0, t2.mx, 0, 1.0 / t2.s, t2.my, 0, 0, 1};
    double tmp[9], Hu[9];
    mat3_mul(Hh, T1, tmp);
    mat3_mul(T2i, tmp, Hu);
    double inv = 1.0 / (Hu[8] + 1e-8);
    double Hn[9];
    for (int i = 0; i < 9; ++i) { Hn[i] = Hu[i] * inv; Hout[i] = (float)Hn[i]; }
    for (int c = 0; c < 4; ++c) {
        double x, y;
        corner_xy(c, (double)w, (double)h, x, y);
        double qx = Hn[0] * x + Hn[1] * y + Hn[2], qy = Hn[3] * x + Hn[4] * y + Hn[5], qz = Hn[6] * x + Hn[7] * y + Hn[8];
        double sc = fabs(qz) > 1e-8 ? 1.0 / qz : 1.0;
        delta_hat[2 * c] = (float)(qx * sc - x);
        delta_hat[2 * c + 1] = (float)(qy * sc - y);
    }
    return m;
}
