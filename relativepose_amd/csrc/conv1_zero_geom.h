// conv1's zero-unit test (RELPOSE_TUNE_CONV1_ZERO): which occupancy words and bits an 8 x 32 pixel tile of A1 depends on.
// Plain C++ (host and device): csrc/scnet.hip includes it, tests/host/conv1_zero_geom_main.cpp checks it exhaustively on the CPU.
#pragma once
#include "rp_math.h"                                // RP_HD: __host__ __device__ under hipcc, inline on the host

constexpr int C1Z_RS = 224;                         // X0 / A1 side
constexpr int C1Z_BLK = 8, C1Z_NB = C1Z_RS / C1Z_BLK;   // occupancy block (pixels), blocks per image side (a bit each, 28)
constexpr int C1Z_TW = 32, C1Z_TH = 8;              // conv1_mfma_kernel's tile: 8 rows x 32 columns
constexpr int C1Z_TPR = C1Z_RS / C1Z_TW;            // tiles per row of tiles (7)
constexpr int C1Z_TILES = C1Z_TPR * (C1Z_RS / C1Z_TH);   // tiles per image (196)

// Tile `tile` (row-major, 7 per row) reads X0 rows 8 by - 1 .. 8 by + 8 and columns 32 tx - 1 .. 32 tx + 32 (its pixels plus the one-pixel
// halo of the 3 x 3 conv), clipped to the image: inside block rows [by0, by1) = by - 1 .. by + 1 and block columns 4 tx - 1 .. 4 tx + 4
// (the bits of `mask`), conservative by up to 7 pixels per side.
struct C1zRange { int by0, by1; unsigned mask; };
RP_HD C1zRange c1z_range(int tile) {
    const int by = tile / C1Z_TPR, tx = tile - by * C1Z_TPR;
    C1zRange r;
    r.by0 = by - 1 < 0 ? 0 : by - 1;
    r.by1 = by + 2 > C1Z_NB ? C1Z_NB : by + 2;
    const int bx0 = 4 * tx - 1 < 0 ? 0 : 4 * tx - 1, bx1 = 4 * tx + 5 > C1Z_NB ? C1Z_NB : 4 * tx + 5;
    r.mask = ((1u << bx1) - 1u) & ~((1u << bx0) - 1u);
    return r;
}

// Index of the occupancy word of (image, stream q, block row) and of the state byte of (image, stream q, tile).
RP_HD long long c1z_word(int img, int q, int by) { return ((long long)img * 6 + q) * C1Z_NB + by; }
RP_HD long long c1z_byte(int img, int q, int tile) { return ((long long)img * 6 + q) * C1Z_TILES + tile; }
