// What pg_frame_metrics_val adds to a tile (posegen_amd/csrc/pg_metrics_plan.h: resample_tap, resample_blend, overlap, valid_ok,
// slot_offset and slot_bytes at SUMS_VAL) on the CPU under ASan + UBSan.  A tile's tap tables, the low-resolution axis and the slot buffer
// are vectors of this program: a tap that names a texel outside the low-resolution frame, a table entry past the staged rows, or a
// 12-wide slot outside its buffer shows as a heap overflow; a weight outside [0, 1], a tap that runs backwards, a count that differs
// from the pixels counted one by one, or a slot written twice as a failed check.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc metrics_resample_asan.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_metrics_plan.h"

namespace {

using namespace pgsp;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

// one axis n_in -> n_out, the box = the whole axis: what every tile puts into its table, as the kernel fills it
void check_axis(int n_in, int n_out) {
    std::vector<float> lo((size_t)n_in);
    for (int i = 0; i < n_in; ++i) lo[(size_t)i] = (float)(i % 7) * 0.125f + 0.0625f;
    std::vector<char> seen((size_t)n_out, 0);
    const int nt = tiles_along(n_out);
    int last_i0 = 0;
    for (int t = 0; t < nt; ++t) {
        const Span s = tile_span(n_out, t);
        std::vector<Tap> tab((size_t)s.sn);                          // the tile's table: one entry per staged pixel
        for (int i = 0; i < s.sn; ++i) tab.data()[i] = resample_tap(n_in, n_out, s.s0 + i);
        for (int i = 0; i < s.sn; ++i) {
            const Tap tp = tab.data()[i];
            CHECK(tp.i0 >= 0 && tp.i0 <= n_in - 1 && tp.i1 >= tp.i0 && tp.i1 <= tp.i0 + 1 && tp.i1 <= n_in - 1);
            CHECK(tp.i1 == tp.i0 + (tp.i0 < n_in - 1 ? 1 : 0));
            CHECK(tp.l1 >= 0.0 && tp.l1 <= 1.0);
            const float a = lo.data()[tp.i0], b = lo.data()[tp.i1];    // ASan: the texels are inside the axis
            const float u = resample_blend(a, b, a, b, tp.l1, 0.0);
            CHECK(u >= (a < b ? a : b) && u <= (a < b ? b : a));
            CHECK(resample_blend(a, a, b, b, 0.0, tp.l1) == u);       // the other axis blends the same way
            if (n_in == n_out) CHECK(tp.i0 == s.s0 + i && tp.l1 == 0.0 && u == a);
            if (n_in == 1) CHECK(u == a);
            if (i < s.own) {                                          // own pixels walk the axis once, in order: i0 never runs backwards
                CHECK(seen.data()[s.s0 + i]++ == 0);
                CHECK(tp.i0 >= last_i0);
                last_i0 = tp.i0;
            }
        }
    }
    for (char c : seen) CHECK(c == 1);
    CHECK(resample_tap(n_in, n_out, 0).i0 == 0 && resample_tap(n_in, n_out, n_out - 1).i1 == n_in - 1);
}

// a w x h box with a valid rectangle (box-relative, it may reach outside): every 12-wide slot inside the buffer and written once, and
// the counts from the spans equal the pixels counted one by one
void check_slots(int w, int h, int vx0, int vy0, int vx1, int vy1) {
    const int ntx = tiles_along(w), nty = tiles_along(h);
    std::vector<char> slots(slot_bytes(w, h, SUMS_VAL), 0);
    CHECK(slots.size() == (size_t)ntx * nty * SUMS_VAL * sizeof(double));
    long n_valid = 0, n_valid_map = 0;
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            const Span xs = tile_span(w, tx), ys = tile_span(h, ty);
            const size_t off = slot_offset(ntx, tx, ty, SUMS_VAL) * sizeof(double);
            for (size_t b = 0; b < SUMS_VAL * sizeof(double); ++b) CHECK(slots.data()[off + b]++ == 0);
            n_valid += (long)overlap(xs.s0, xs.s0 + xs.own, vx0, vx1) * overlap(ys.s0, ys.s0 + ys.own, vy0, vy1);
            if (xs.map > 0 && ys.map > 0)
                n_valid_map += (long)overlap(xs.s0 + WIN / 2, xs.s0 + WIN / 2 + xs.map, vx0, vx1) *
                               overlap(ys.s0 + WIN / 2, ys.s0 + WIN / 2 + ys.map, vy0, vy1);
        }
    for (char c : slots) CHECK(c == 1);
    long want = 0, want_map = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const bool in = x >= vx0 && x < vx1 && y >= vy0 && y < vy1;
            want += in;
            want_map += in && w > HALO && h > HALO && x >= WIN / 2 && x < w - WIN / 2 && y >= WIN / 2 && y < h - WIN / 2;
        }
    CHECK(n_valid == want && n_valid_map == want_map);
}

void check_valid_ok() {
    const int H = 50, W = 37;
    long good = 0;
    for (int x0 = -2; x0 <= W + 2; ++x0)
        for (int x1 = -2; x1 <= W + 2; x1 += 3)
            for (int y0 = -2; y0 <= H + 2; y0 += 5)
                for (int y1 = -2; y1 <= H + 2; y1 += 7) {
                    const int32_t v[4] = {x0, y0, x1, y1};
                    const bool want = x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H && x1 >= x0 && y1 >= y0;
                    CHECK(valid_ok(v, H, W) == want);
                    good += want;
                }
    CHECK(good > 100);
    const int32_t empty[4] = {5, 5, 5, 5}, big[4] = {0, 0, 0x7fffffff, 0x7fffffff};
    CHECK(valid_ok(empty, H, W) && !valid_ok(big, H, W));
}

}  // namespace

int main() {
    static_assert(SUMS_VAL == SUMS + 4, "the valid sums follow the eight");
    long pairs = 0;
    for (int n_out = 1; n_out <= 130; ++n_out)
        for (int n_in = 1; n_in <= n_out; ++n_in) { check_axis(n_in, n_out); ++pairs; }
    check_axis(500, 1000); check_axis(1, 4096); pairs += 2;
    long boxes = 0;
    const int lens[] = {1, 7, 10, 11, 12, 41, 42, 43, 74, 75, 101, 3 * TILE + HALO + 1};
    for (int w : lens)
        for (int h : lens) {
            check_slots(w, h, 0, 0, w, h);                           // the box itself
            check_slots(w, h, -3, 2, w / 2, h + 4);                  // straddling two edges
            check_slots(w, h, w, 0, w + 5, h);                       // beside the box
            check_slots(w, h, w / 3, h / 3, w / 3, h);               // empty
            check_slots(w, h, TILE, TILE + WIN / 2, 2 * TILE, 2 * TILE + WIN / 2);      // edges on tile seams
            boxes += 5;
        }
    check_slots(1000, 1000, 100, 50, 900, 1000); check_slots(1, 4096, 0, 7, 1, 4000); boxes += 2;
    check_valid_ok();
    std::printf("%ld axis pairs and %ld boxes clean under ASan/UBSan\n", pairs, boxes);
    return 0;
}
