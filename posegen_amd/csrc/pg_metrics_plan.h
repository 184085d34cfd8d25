// pg_metrics_plan.h -- the box and tile arithmetic of pg_frame_metrics and pg_frame_metrics_val (pg_metrics.hip, DESIGN.md 2.8,
// 2.8b): the check of a box against its frame, the grid of tiles over the box, what a tile stages, which pixels' squared errors
// and which map pixels it owns, where its partial sums go, and the per-axis taps and the blend of the bilinear resampling.
// Free of HIP calls, like pg_frames_plan.h, so that it compiles into plain C++ programs (tools/sanitize/metrics_plan_asan.cpp and
// metrics_resample_asan.cpp, built with the address and undefined-behaviour sanitisers); the kernel runs the same functions on
// the device.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PG_METRICS_HD __host__ __device__
#else
#define PG_METRICS_HD
#endif

namespace pgsp {

constexpr int WIN = 11;                  // the Gaussian window of pytorch_msssim (window_size = 11, valid convolution)
constexpr int HALO = WIN - 1;
constexpr int TILE = 32;                 // map pixels of a tile along each axis
constexpr int STAGE = TILE + HALO;       // box pixels a tile stages along each axis
constexpr int SUMS = 8;                  // (n, se, n_fg, se_fg, n_map, ssim, n_fg_map, ssim_fg)
constexpr int SUMS_VAL = 12;             // pg_frame_metrics_val: those and (n_valid, se_valid, n_valid_map, ssim_valid)
// The float32 taps of pytorch_msssim's gaussian(11, 1.5), bit for bit (tests/golden/frame_metrics.npz holds what that function
// returns; tests/test_frame_metrics_ref.py compares).  The 2-D window is their outer product, formed in double.
constexpr float TAPS[WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                             0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

// A box (x0, y0, x1, y1), top-left inclusive and bottom-right exclusive, inside an H x W frame and not empty
PG_METRICS_HD inline bool box_ok(const int32_t box[4], int H, int W) {
    return box[0] >= 0 && box[1] >= 0 && box[0] < box[2] && box[1] < box[3] && box[2] <= W && box[3] <= H;
}

// Tiles along an axis of `len` box pixels: the map has len - HALO pixels there, TILE per tile; a box below the window has no map
// and one tile, which still owns the box's squared errors.
PG_METRICS_HD inline int tiles_along(int len) { return len > HALO ? (len - HALO + TILE - 1) / TILE : 1; }

struct Span {
    int s0, sn;      // staged box pixels [s0, s0 + sn), sn <= STAGE
    int own;         // the first `own` of them are this tile's for the squared error: every box pixel belongs to one tile
    int map;         // map pixels s0 .. s0 + map (<= TILE): map pixel i has its window over staged pixels [i, i + WIN)
};

// Tile t of tiles_along(len) along one axis (box-relative pixels)
PG_METRICS_HD inline Span tile_span(int len, int t) {
    const int nt = tiles_along(len);
    Span s;
    s.s0 = t * TILE;
    s.sn = len - s.s0 < STAGE ? len - s.s0 : STAGE;
    s.own = t == nt - 1 ? len - s.s0 : TILE;
    const int mlen = len > HALO ? len - HALO : 0;
    s.map = mlen - s.s0 < TILE ? mlen - s.s0 : TILE;
    if (s.map < 0) s.map = 0;
    return s;
}

// Partial sums of tile (tx, ty): n doubles at this offset of the slot buffer, n = SUMS, or SUMS_VAL with a valid rectangle
PG_METRICS_HD inline size_t slot_offset(int ntx, int tx, int ty, int n) { return ((size_t)ty * ntx + tx) * n; }
inline size_t slot_bytes(int w, int h, int n) { return (size_t)tiles_along(w) * tiles_along(h) * n * sizeof(double); }

// ---- pg_frame_metrics_val: the valid rectangle and the bilinear resampling of a low-resolution frame ----------------
// A valid rectangle (vx0, vy0, vx1, vy1) inside an H x W frame; it may be empty (x0 == x1 or y0 == y1), unlike a box
PG_METRICS_HD inline bool valid_ok(const int32_t v[4], int H, int W) {
    return v[0] >= 0 && v[1] >= 0 && v[0] <= v[2] && v[1] <= v[3] && v[2] <= W && v[3] <= H;
}
// |[a0, a1) n [b0, b1)|
PG_METRICS_HD inline int overlap(int a0, int a1, int b0, int b1) {
    const int lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0;
}

// Output pixel d of an axis resampled n_in -> n_out (1 <= n_in <= n_out): F.interpolate(mode='bilinear', align_corners=False)
// with the index arithmetic in double.  Texels i0 and i1 (= i0 at the last texel), weights 1 - l1 and l1.
struct Tap {
    int i0, i1;
    double l1;
};
PG_METRICS_HD inline Tap resample_tap(int n_in, int n_out, int d) {
#pragma clang fp contract(off)
    double src = ((double)n_in / (double)n_out) * ((double)d + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > n_in - 1) t.i0 = n_in - 1;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = src - (double)t.i0;
    return t;
}
// The upsampled value from the four texels a (y0, x0), b (y0, x1), c (y1, x0), d (y1, x1): every product and sum rounded on its
// own in double, the result rounded once to float32
PG_METRICS_HD inline float resample_blend(double a, double b, double c, double d, double lx1, double ly1) {
#pragma clang fp contract(off)
    const double lx0 = 1.0 - lx1, ly0 = 1.0 - ly1;
    const double top = lx0 * a + lx1 * b;
    const double bot = lx0 * c + lx1 * d;
    return (float)(ly0 * top + ly1 * bot);
}

}  // namespace pgsp
