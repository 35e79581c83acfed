// tile_shape.h -- the tiles of the image-space kernels (denoise.hip, denoise_variance.hip, upsample.hip, temporal.hip, lightmap.hip;
// the device side of the walk: image_kernels.h) as the host entries and the kernels both see them.  A 256-thread block covers a tile
// of 64 x 4 pixels, one pixel per lane and one wave per row; tiles are numbered (view, tile row, tile column), and a block walks them
// with the stride of its grid.  Plain integers and no HIP type, so that tests/cpp/tile_walk.cpp and tests/cpp/plane_checks.cpp build
// it with the host compiler; constexpr, which under hipcc makes a function host and device code.  Nothing wraps for a frame the
// entries accept: n_views * width * height < 2^32 (MIPT_BATCH_MAX_PIXELS).
#pragma once
#include <cstdint>

namespace mipt {

constexpr uint32_t kTileW = 64, kTileH = 4;

// blocks per launch; past it a block walks more than one tile
constexpr uint32_t kFrameMaxGrid = 1u << 20;                 // denoise.hip, denoise_variance.hip, upsample.hip, temporal.hip
constexpr uint32_t kAtlasMaxGrid = 1u << 16;                 // lightmap.hip: the filter and the dilation

// tiles per row / per column of a view (the quotient first: width + 63 would wrap for the widest row)
constexpr uint32_t tiles_across(uint32_t width) { return width / kTileW + (width % kTileW != 0u ? 1u : 0u); }
constexpr uint32_t tiles_down(uint32_t height) { return height / kTileH + (height % kTileH != 0u ? 1u : 0u); }
// tiles of a launch over n_views views.  One view's count is at most 2^30 (a column one pixel wide), so it fits the atlas kernels'
// 32-bit walk and tile_pixel's 32-bit per_view.
constexpr unsigned long long tile_count(uint32_t tiles_x, uint32_t tiles_y, uint32_t n_views) { return (unsigned long long)tiles_x * tiles_y * n_views; }
constexpr uint32_t tile_grid(unsigned long long n_tiles, uint32_t cap) { return n_tiles < cap ? (uint32_t)n_tiles : cap; }

// The pixel of lane `lane` (0 ... 255) of a tile.  Whether it lies inside the frame is the caller's comparison against width and
// height: a ragged edge tile has lanes that do not.
struct TilePixel { uint32_t view, x, y; };
// tile r of one view: the atlas kernels, whose one view needs no division
constexpr TilePixel tile_texel(uint32_t tiles_x, uint32_t r, uint32_t lane) {
    return TilePixel{0u, (r % tiles_x) * kTileW + (lane & (kTileW - 1u)), (r / tiles_x) * kTileH + lane / kTileW};
}
// tile t of a launch over views of tiles_x * tiles_y tiles each
constexpr TilePixel tile_pixel(uint32_t tiles_x, uint32_t tiles_y, unsigned long long t, uint32_t lane) {
    const uint32_t per_view = tiles_x * tiles_y;
    const TilePixel p = tile_texel(tiles_x, (uint32_t)(t % per_view), lane);
    return TilePixel{(uint32_t)(t / per_view), p.x, p.y};
}

} // namespace mipt
