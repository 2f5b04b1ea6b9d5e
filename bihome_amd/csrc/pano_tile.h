// The canvas tile of the n-frame blends, spelled ONCE for csrc/pano.hip (bh_pano_u8) and csrc/bands.hip (bh_pano_bands_u8): which unit
// of the canvas a thread makes and how many workgroups cover it.  A wavefront's pixels are a compact tile, not a run of one row, because
// a tile is absent from more frames (DESIGN.md section 8 "Panorama" has the figures).
#pragma once

#define PANO_THREADS 256
#ifndef PANO_TILE
#define PANO_TILE 1        // 1: a wavefront makes 8 units x 8 rows of the canvas (a unit: 4 pixels, or 1), a workgroup 32 units x 8 rows - the
#endif                     // compact tile is absent from more frames; 0: mosaic.hip's 64 consecutive units of one row (longer store runs)

// the thread's unit of PX pixels -> (x, y) of its first pixel; false: outside the canvas
template <int PX>
__device__ __forceinline__ bool pano_unit(int Hc, int Wc, int& x, int& y) {
    const unsigned upr = (unsigned)Wc / PX;                                    // units per canvas row
#if PANO_TILE
    const unsigned tiles_x = (upr + 31u) / 32u, by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const unsigned ux = bx * 32u + (threadIdx.x >> 6) * 8u + (threadIdx.x & 7u), uy = by * 8u + ((threadIdx.x >> 3) & 7u);
    if (ux >= upr || uy >= (unsigned)Hc) return false;
    x = (int)ux * PX; y = (int)uy;
#else
    const unsigned u = blockIdx.x * PANO_THREADS + threadIdx.x;
    if (u >= upr * (unsigned)Hc) return false;
    y = (int)(u / upr); x = (int)(u - (unsigned)y * upr) * PX;
#endif
    return true;
}
static unsigned pano_grid_x(int Hc, int Wc, int px) {
    const unsigned upr = (unsigned)Wc / px;
#if PANO_TILE
    return ((upr + 31u) / 32u) * (((unsigned)Hc + 7u) / 8u);
#else
    return (upr * (unsigned)Hc + PANO_THREADS - 1) / PANO_THREADS;
#endif
}
