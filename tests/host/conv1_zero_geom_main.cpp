// Host check of conv1's zero-unit geometry (csrc/conv1_zero_geom.h, the function conv1_mfma_kernel calls): for every tile the block rows
// and the column mask must be exactly the blocks stated in DESIGN.md 4.1 -- rows by - 1 .. by + 1, columns 4 tx - 1 .. 4 tx + 4, clipped
// to the image -- they must cover every X0 pixel the tile's 3 x 3 convolution reads, and every word and state-byte index of
// 196 tiles x 6 streams x n images must lie inside its array.  Built with -fsanitize=address,undefined: the arrays are real heap blocks
// of exactly the size the library allocates, written and read through those indices.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv1_zero_geom.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

int main() {
    const int n = 6;
    std::vector<unsigned> occ((size_t)n * 6 * C1Z_NB, 0u);
    std::vector<unsigned char> state((size_t)n * 6 * C1Z_TILES, 0);
    CHECK(C1Z_TILES == 196 && C1Z_NB == 28 && C1Z_TPR == 7);
    long long units = 0;
    for (int tile = 0; tile < C1Z_TILES; ++tile) {
        const C1zRange r = c1z_range(tile);
        const int by = tile / 7, tx = tile % 7;
        // the stated geometry, block by block
        CHECK(r.by0 >= 0 && r.by0 < r.by1 && r.by1 <= C1Z_NB);
        for (int b = 0; b < 32; ++b) {
            const bool row_in = b >= by - 1 && b <= by + 1 && b < C1Z_NB;
            CHECK((b >= r.by0 && b < r.by1) == row_in);
            const bool col_in = b >= 4 * tx - 1 && b <= 4 * tx + 4 && b < C1Z_NB;
            CHECK((((r.mask >> b) & 1u) != 0u) == col_in);
        }
        // every pixel the tile reads (its 8 x 32 pixels and the one-pixel halo, inside the image) lies in a tested block
        for (int y = 8 * by - 1; y <= 8 * by + 8; ++y)
            for (int x = 32 * tx - 1; x <= 32 * tx + 32; ++x) {
                if (y < 0 || y >= C1Z_RS || x < 0 || x >= C1Z_RS) continue;
                CHECK(y / C1Z_BLK >= r.by0 && y / C1Z_BLK < r.by1);
                CHECK((r.mask >> (x / C1Z_BLK)) & 1u);
            }
        // ... and the range is conservative by at most 7 pixels per side
        CHECK(8 * by - 1 - 8 * r.by0 <= 7 && 8 * r.by1 - 1 - (8 * by + 8) <= 7);
        // indices: every image and stream, through real arrays
        for (int img = 0; img < n; ++img)
            for (int q = 0; q < 6; ++q) {
                unsigned any = 0u;
                for (int b = r.by0; b < r.by1; ++b) {
                    const long long w = c1z_word(img, q, b);
                    CHECK(w >= 0 && w < (long long)occ.size());
                    any |= occ.data()[w] & r.mask;
                }
                const long long s = c1z_byte(img, q, tile);
                CHECK(s >= 0 && s < (long long)state.size());
                CHECK(state.data()[s] == 0);          // each byte belongs to one (image, stream, tile)
                state.data()[s] = any ? 0 : 1;
                ++units;
            }
    }
    CHECK(units == (long long)state.size());
    for (unsigned char b : state) CHECK(b == 1);
    std::printf("conv1_zero_geom ok: %lld units\n", units);
    return 0;
}
