// What pg_frame_metrics decides about a box before and inside its launch (posegen_amd/csrc/pg_metrics_plan.h: box_ok, tiles_along,
// tile_span, slot_offset) on the CPU under ASan + UBSan.  The box, its SSIM map, a tile's staged pixels and the slot buffer are
// vectors of this program, so a tile that reaches outside the box or the stage, or a slot outside the buffer, shows as a heap
// overflow; a pixel owned twice or never as a failed check.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc metrics_plan_asan.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_metrics_plan.h"

namespace {

using namespace pgsp;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

// one w x h box: every box pixel owned once, every map pixel computed once from staged pixels only, every slot written once
void check_box(int w, int h) {
    const int ntx = tiles_along(w), nty = tiles_along(h);
    const int mw = w > HALO ? w - HALO : 0, mh = h > HALO ? h - HALO : 0;
    const bool has_map = mw > 0 && mh > 0;
    std::vector<char> owned((size_t)w * h, 0), mapped((size_t)mw * mh, 0);
    std::vector<char> slots(slot_bytes(w, h, SUMS), 0);
    CHECK(slots.size() == (size_t)ntx * nty * SUMS * sizeof(double));
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            const Span xs = tile_span(w, tx), ys = tile_span(h, ty);
            CHECK(xs.s0 >= 0 && xs.sn >= 1 && xs.sn <= STAGE && xs.s0 + xs.sn <= w);
            CHECK(ys.s0 >= 0 && ys.sn >= 1 && ys.sn <= STAGE && ys.s0 + ys.sn <= h);
            CHECK(xs.own >= 1 && xs.own <= xs.sn && ys.own >= 1 && ys.own <= ys.sn);
            CHECK(xs.map >= 0 && xs.map <= TILE && ys.map >= 0 && ys.map <= TILE);
            std::vector<char> stage((size_t)xs.sn * ys.sn, 1);              // what the tile has staged of the box
            for (int r = 0; r < ys.own; ++r)
                for (int c = 0; c < xs.own; ++c) CHECK(owned.data()[(size_t)(ys.s0 + r) * w + xs.s0 + c]++ == 0);
            if (xs.map > 0 && ys.map > 0) {
                CHECK(has_map);
                for (int i = 0; i < ys.map; ++i)
                    for (int j = 0; j < xs.map; ++j) {
                        CHECK(mapped.data()[(size_t)(ys.s0 + i) * mw + xs.s0 + j]++ == 0);
                        // the window's corners and its centre (the masked variant's weight) are staged pixels
                        CHECK(stage.data()[(size_t)i * xs.sn + j] == 1);
                        CHECK(stage.data()[(size_t)(i + WIN - 1) * xs.sn + j + WIN - 1] == 1);
                        CHECK(stage.data()[(size_t)(i + WIN / 2) * xs.sn + j + WIN / 2] == 1);
                    }
            }
            const size_t off = slot_offset(ntx, tx, ty, SUMS) * sizeof(double);
            for (size_t b = 0; b < SUMS * sizeof(double); ++b) CHECK(slots.data()[off + b]++ == 0);
        }
    for (char c : owned) CHECK(c == 1);
    for (char c : mapped) CHECK(c == 1);
    for (char c : slots) CHECK(c == 1);
}

void check_box_ok() {
    const int H = 50, W = 37;
    long good = 0;
    for (int x0 = -2; x0 <= W + 2; ++x0)
        for (int x1 = -2; x1 <= W + 2; x1 += 3)
            for (int y0 = -2; y0 <= H + 2; y0 += 5)
                for (int y1 = -2; y1 <= H + 2; y1 += 7) {
                    const int32_t box[4] = {x0, y0, x1, y1};
                    const bool want = x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H && x1 > x0 && y1 > y0;
                    CHECK(box_ok(box, H, W) == want);
                    good += want;
                }
    CHECK(good > 100);
    const int32_t big[4] = {0, 0, 0x7fffffff, 0x7fffffff}, neg[4] = {(int32_t)0x80000000, 0, 1, 1};
    CHECK(!box_ok(big, H, W) && !box_ok(neg, H, W));
}

}  // namespace

int main() {
    static_assert(STAGE == TILE + WIN - 1, "a tile stages its map pixels' windows");
    double sum = 0.0;
    for (int t = 0; t < WIN; ++t) { CHECK(TAPS[t] == TAPS[WIN - 1 - t]); sum += (double)TAPS[t]; }
    CHECK(sum > 1.0 - 1e-6 && sum < 1.0 + 1e-6);
    long boxes = 0;
    const int lens[] = {1, 2, 9, 10, 11, 12, 13, 41, 42, 43, 44, 73, 74, 75, 76, 100, 3 * TILE + HALO, 3 * TILE + HALO + 1, 131};
    for (int w : lens)
        for (int h : lens) { check_box(w, h); ++boxes; }
    for (int w = 1; w <= 4 * TILE + HALO + 2; ++w) { check_box(w, 11); check_box(11, w); check_box(w, 7); boxes += 3; }
    check_box(1000, 1000); check_box(1, 4096); check_box(4096, 1); boxes += 3;
    check_box_ok();
    std::printf("%ld boxes clean under ASan/UBSan\n", boxes);
    return 0;
}
