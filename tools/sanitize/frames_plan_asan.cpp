// What pg_render_frames decides on the host (posegen_amd/csrc/pg_frames_plan.h: plan_frames, partition_frames, FrameLayout) on the
// CPU under ASan + UBSan.  The workers' range buffers are vectors of this program with one byte per ray, so a run that is placed
// outside its worker's buffer shows as a heap overflow and two runs that share rays as a failed check.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc frames_plan_asan.cpp
#include <cstdio>
#include <cstdlib>

#include "pg_frames_plan.h"

namespace {

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

uint32_t g_seed = 1;
long g_cut_runs = 0;     // runs of cut frames seen: the sweep has to reach the range buffers
uint32_t draw() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// ray counts of F frames: 0, below chunk, whole multiples, non-multiples of chunk, small and large
std::vector<int64_t> ray_counts(int F, int chunk, int variant) {
    const int64_t c = chunk;
    const int64_t kinds[] = {0, c - 1, c / 2, c, c + 1, 3 * c + c / 3 + 1, 7 * c, 20 * c + 5, (int64_t)(draw() % (40 * c + 7))};
    std::vector<int64_t> n(F);
    for (int f = 0; f < F; ++f) n[f] = variant == 0 ? kinds[f % 9] : variant == 1 ? 9 * c + 3 : kinds[draw() % 9];
    return n;
}

void check_plan(const std::vector<int64_t>& n_rays, int G, int chunk) {
    const int F = (int)n_rays.size();
    std::vector<FrameTask> tasks;
    plan_frames(n_rays, G, chunk, &tasks);
    // every frame's [0, n) exactly once and in order, every cut on a multiple of chunk, the owner = the worker of the first run
    std::vector<int64_t> reached(F, 0);
    std::vector<int> runs(F, 0), owner(F, -1);
    for (const FrameTask& tk : tasks) {
        CHECK(tk.frame >= 0 && tk.frame < F && tk.worker >= 0 && tk.worker < G && tk.owner >= 0 && tk.owner < G);
        const int64_t n = n_rays[tk.frame];
        CHECK(tk.r0 == reached[tk.frame] && tk.r1 >= tk.r0 && tk.r1 <= n);
        CHECK(tk.r1 > tk.r0 || n == 0);
        CHECK(tk.r0 % chunk == 0 && (tk.r1 % chunk == 0 || tk.r1 == n));
        if (runs[tk.frame]++ == 0) owner[tk.frame] = tk.worker;
        CHECK(tk.owner == owner[tk.frame]);
        reached[tk.frame] = tk.r1;
    }
    for (int f = 0; f < F; ++f) {
        CHECK(reached[f] == n_rays[f] && runs[f] >= 1);
        CHECK(n_rays[f] > 0 || runs[f] == 1);           // a frame with no rays: one empty task
    }
    // the range buffers: a worker's runs are disjoint and end within its total; whole frames take no room
    const FramePartition p = partition_frames(tasks, n_rays, G);
    CHECK((int)p.composes.size() == G && (int)p.part_rays.size() == G && p.part_off.size() == tasks.size());
    std::vector<std::vector<char>> buf(G);
    for (int k = 0; k < G; ++k) buf[k].assign(p.part_rays[k], 0);
    std::vector<char> composes(G, 0);
    bool split = false;
    for (size_t t = 0; t < tasks.size(); ++t) {
        const FrameTask& tk = tasks[t];
        const bool whole = task_whole(tk, n_rays);
        CHECK(whole == (runs[tk.frame] == 1));
        composes[whole ? tk.worker : tk.owner] = 1;
        if (whole) { CHECK(p.part_off[t] == 0); continue; }
        split = true;
        ++g_cut_runs;
        const size_t len = (size_t)(tk.r1 - tk.r0);
        CHECK(p.part_off[t] + len <= p.part_rays[tk.worker]);
        for (size_t i = 0; i < len; ++i) CHECK(buf[tk.worker].data()[p.part_off[t] + i]++ == 0);
    }
    CHECK(split == p.split);
    for (int k = 0; k < G; ++k) {
        CHECK(composes[k] == p.composes[k]);
        for (char c : buf[k]) CHECK(c == 1);            // (and nothing of a buffer is left over)
    }
}

void check_layout(size_t hw) {
    const FrameLayout lay{hw};
    const FrameRegion r[4] = {lay.rgb(), lay.disp(), lay.acc(), lay.rgb8()};
    CHECK(r[0].off == 0 && r[0].bytes == hw * 3 * sizeof(float) && r[1].bytes == hw * sizeof(float) && r[2].bytes == r[1].bytes && r[3].bytes == hw * 3);
    size_t sum = 0;
    for (int i = 0; i < 4; ++i) {
        CHECK(r[i].off % sizeof(float) == 0);
        CHECK(r[i].off + r[i].bytes <= (i < 3 ? r[i + 1].off : lay.bytes()));
        sum += i < 3 ? r[i].bytes : (r[i].bytes + 255) / 256 * 256;     // (the uint8 frame's room is rounded up to 256 bytes)
    }
    CHECK(sum == lay.bytes() && lay.bytes() % sizeof(float) == 0);
}

}  // namespace

int main() {
    long plans = 0;
    for (int chunk : {1, 64, 1024})
        for (int F = 0; F <= 7; ++F)
            for (int G = 1; G <= 8; ++G)
                for (int variant = 0; variant < 6; ++variant, ++plans) check_plan(ray_counts(F, chunk, variant), G, chunk);
    for (size_t hw : {(size_t)0, (size_t)1, (size_t)85, (size_t)48 * 48, (size_t)96 * 96, (size_t)512 * 512, (size_t)1 << 31}) check_layout(hw);
    CHECK(g_cut_runs > plans);
    std::printf("%ld frame plans clean under ASan/UBSan\n", plans);
    return 0;
}
