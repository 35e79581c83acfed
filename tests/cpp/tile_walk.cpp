// tile_walk.cpp -- the tile arithmetic of the image-space kernels (rust_ray_tracing_amd/csrc/tile_shape.h) under AddressSanitizer +
// UBSan on the CPU, without HIP and without libmipt.so.  Widths 1, 63, 64, 65, 129 by heights 1, 3, 4, 5, 9 with 1 and 3 views are
// walked as a launch walks them -- every block of a grid, tile after tile with the grid's stride, lanes 0 ... 255 -- on a grid that
// holds every tile and on capped ones, and each in-frame pixel of each view must be met exactly once, no index reaching n_views *
// width * height; the atlas decode walks the one-view frames the same way.  Then the largest operands -- 2^32 - 1 pixels as one row,
// as one column, and as 2^20 + 700 views of 2x1 -- against 128-bit arithmetic, and tile_grid around both caps.
// Built and run by tests/test_cpp_host.py::test_tile_walk_under_asan_ubsan.
#include "../../rust_ray_tracing_amd/csrc/tile_shape.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

using namespace mipt;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

u64 g_width, g_height, g_views, g_grid;                  // the case a failure names
#define CHECK(cond)                                                                                                              \
    do {                                                                                                                        \
        if (!(cond)) {                                                                                                          \
            fprintf(stderr, "tile_walk: line %d: %s (%llu views of %llux%llu, grid %llu)\n", __LINE__, #cond, g_views, g_width, g_height, g_grid); \
            exit(1);                                                                                                            \
        }                                                                                                                       \
    } while (0)

const uint32_t kLanes = kTileW * kTileH;

// a launch of `grid` blocks over the frame; atlas: the one-view decode on a 32-bit walk
void walk(uint32_t width, uint32_t height, uint32_t n_views, uint32_t grid, bool atlas) {
    g_width = width; g_height = height; g_views = n_views; g_grid = grid;
    const uint32_t tiles_x = tiles_across(width), tiles_y = tiles_down(height);
    CHECK((u64)tiles_x * kTileW >= width && (u64)(tiles_x - 1u) * kTileW < width);
    CHECK((u64)tiles_y * kTileH >= height && (u64)(tiles_y - 1u) * kTileH < height);
    const u64 n_tiles = tile_count(tiles_x, tiles_y, n_views), n_pixels = (u64)n_views * width * height;
    CHECK(n_tiles == (u64)tiles_x * tiles_y * n_views);
    std::vector<unsigned> met(n_pixels, 0u);
    u64 tiles_walked = 0;
    for (uint32_t block = 0; block < grid; block++)
        for (u64 t = block; t < n_tiles; t += grid, tiles_walked++)
            for (uint32_t lane = 0; lane < kLanes; lane++) {
                const TilePixel p = atlas ? tile_texel(tiles_x, (uint32_t)t, lane) : tile_pixel(tiles_x, tiles_y, t, lane);
                CHECK(p.view < n_views);
                if (p.x >= width || p.y >= height) continue;             // the caller's comparison: a ragged edge tile
                const u64 i = (u64)p.view * width * height + ((u64)p.y * width + p.x);
                CHECK(i < n_pixels);
                met[i]++;
            }
    CHECK(tiles_walked == n_tiles);
    for (u64 i = 0; i < n_pixels; i++) CHECK(met[i] == 1u);
}

// tile t, lane `lane` against the decode written out in 128 bits
void decode_is(uint32_t tiles_x, uint32_t tiles_y, u64 t, uint32_t lane) {
    const u128 per_view = (u128)tiles_x * tiles_y, r = (u128)t % per_view;
    const u128 x = (r % tiles_x) * kTileW + lane % kTileW, y = (r / tiles_x) * kTileH + lane / kTileW;
    const TilePixel p = tile_pixel(tiles_x, tiles_y, t, lane);
    CHECK((u128)p.view == (u128)t / per_view && (u128)p.x == x && (u128)p.y == y);
    if (t < per_view) {
        const TilePixel a = tile_texel(tiles_x, (uint32_t)t, lane);
        CHECK(a.view == 0u && a.x == p.x && a.y == p.y);
    }
}

void largest(uint32_t width, uint32_t height, uint32_t n_views) {
    g_width = width; g_height = height; g_views = n_views; g_grid = 0;
    const uint32_t tiles_x = tiles_across(width), tiles_y = tiles_down(height);
    CHECK((u128)tiles_x == ((u128)width + kTileW - 1u) / kTileW && (u128)tiles_y == ((u128)height + kTileH - 1u) / kTileH);
    const u64 n_tiles = tile_count(tiles_x, tiles_y, n_views);
    CHECK((u128)n_tiles == (u128)tiles_x * tiles_y * n_views);
    CHECK((u64)tiles_x * tiles_y < (1ull << 31));                       // one view: the lightmap's 32-bit walk, tile_pixel's per_view
    const u64 per_view = (u64)tiles_x * tiles_y;
    const u64 some[] = {0, 1, per_view - 1, per_view, n_tiles / 2, n_tiles - per_view, n_tiles - 2, n_tiles - 1};
    for (u64 t : some) {
        if (t >= n_tiles) continue;
        for (uint32_t lane : {0u, 1u, 63u, 64u, 255u}) decode_is(tiles_x, tiles_y, t, lane);
    }
    // the frame's last pixel is in the last tile, and its index is the last one
    bool found = false;
    for (uint32_t lane = 0; lane < kLanes; lane++) {
        const TilePixel p = tile_pixel(tiles_x, tiles_y, n_tiles - 1, lane);
        CHECK(p.view == n_views - 1u);
        if (p.x >= width || p.y >= height) continue;
        const u128 i = (u128)p.view * width * height + ((u128)p.y * width + p.x);
        CHECK(i < (u128)n_views * width * height);
        found = found || i == (u128)n_views * width * height - 1;
    }
    CHECK(found);
}

void grids() {
    g_width = g_height = g_views = 0;
    for (uint32_t cap : {kFrameMaxGrid, kAtlasMaxGrid, 1u, 7u}) {
        g_grid = cap;
        CHECK(tile_grid(cap - 1ull, cap) == cap - 1u && tile_grid(cap, cap) == cap && tile_grid(cap + 1ull, cap) == cap);
        CHECK(tile_grid(1, cap) == 1u && tile_grid(~0ull, cap) == cap && tile_grid(1ull << 32, cap) == cap);
    }
    CHECK(kFrameMaxGrid == 1u << 20 && kAtlasMaxGrid == 1u << 16 && kLanes == 256u);
}

} // namespace

int main() {
    for (uint32_t width : {1u, 63u, 64u, 65u, 129u})
        for (uint32_t height : {1u, 3u, 4u, 5u, 9u})
            for (uint32_t n_views : {1u, 3u}) {
                const u64 n_tiles = tile_count(tiles_across(width), tiles_down(height), n_views);
                for (uint32_t cap : {kFrameMaxGrid, 1u, 2u, 5u}) {       // every tile its own block; then blocks that walk several
                    walk(width, height, n_views, tile_grid(n_tiles, cap), false);
                    if (n_views == 1u) walk(width, height, 1u, tile_grid(n_tiles, cap), true);
                }
            }
    largest(0xffffffffu, 1u, 1u);
    largest(1u, 0xffffffffu, 1u);
    largest(2u, 1u, (1u << 20) + 700u);
    grids();
    printf("tile_walk ok\n");
    return 0;
}
