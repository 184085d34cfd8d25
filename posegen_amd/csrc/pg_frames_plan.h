// pg_frames_plan.h -- what pg_render_frames decides on the host before its first launch: the work plan of a frame batch over the
// workers, the partition of the cut frames' ray ranges over the workers' range buffers, and the layout of a frame buffer.  Host-only
// and free of HIP calls, like pg_bank.h, so that it compiles into a plain C++ program (tools/sanitize/frames_plan_asan.cpp, built
// with the address and undefined-behaviour sanitisers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct FrameTask { int frame; int64_t r0, r1; int worker; int owner; };

// Work plan of a frame batch on G workers (the call pattern of run_gan.py:2042-2047 is
// 20 frames per call: whole frames alone would leave 3:2 loads on 8 GPUs).  The unit of work is a nanmean
// group (`chunk` consecutive rays of a frame's box).  Frames go to workers whole, largest first, to the
// least loaded worker, as long as they fit under the per-worker target (total rays / G, 2 % slack); the
// frames that do not fit (the tail of a batch with F mod G != 0, or every frame when F < G) are cut into
// contiguous runs of whole groups that fill the least loaded workers up to the target.  Every cut falls
// on a multiple of `chunk`, so every group is rendered exactly as on one device.  A cut frame is composed
// by its owner (the worker of its first run).  Deterministic; dist.plan_tasks is the same algorithm.
inline void plan_frames(const std::vector<int64_t>& n_rays, int G, int chunk, std::vector<FrameTask>* tasks) {
    const int F = (int)n_rays.size();
    tasks->clear();
    if (F == 0) return;
    std::vector<int> order(F);
    for (int f = 0; f < F; ++f) order[f] = f;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_rays[a] > n_rays[b]; });
    int64_t total = 0;
    for (int64_t n : n_rays) total += n > 0 ? n : 0;
    const int64_t target = (total + G - 1) / G;
    std::vector<int64_t> load(G, 0);
    auto least = [&] {
        int w = 0;
        for (int k = 1; k < G; ++k) if (load[k] < load[w]) w = k;
        return w;
    };
    std::vector<int> tail;
    for (int f : order) {
        const int w = least();
        if (n_rays[f] <= chunk || load[w] + n_rays[f] <= target + target / 50) {
            load[w] += n_rays[f] > 0 ? n_rays[f] : 0;
            tasks->push_back({f, 0, n_rays[f] > 0 ? n_rays[f] : 0, w, w});
        } else {
            tail.push_back(f);
        }
    }
    for (int f : tail) {
        const int64_t groups = (n_rays[f] + chunk - 1) / chunk;
        int64_t g = 0;
        int owner = -1;
        while (g < groups) {
            const int w = least();
            const int64_t cap = target - load[w];
            int64_t take = cap > 0 ? (cap + chunk / 2) / chunk : 0;     // nearest whole number of groups
            if (take < 1) take = 1;
            if (take > groups - g) take = groups - g;
            const int64_t rest = groups - g - take;
            if (rest > 0 && rest * chunk <= std::max<int64_t>(chunk, target / 32)) take += rest;   // no sliver of a run for yet another worker
            const int64_t r0 = g * chunk, r1 = std::min((g + take) * chunk, n_rays[f]);
            if (owner < 0) owner = w;
            if (!tasks->empty() && tasks->back().frame == f && tasks->back().worker == w && tasks->back().r1 == r0) tasks->back().r1 = r1;
            else tasks->push_back({f, r0, r1, w, owner});
            load[w] += r1 - r0;
            g += take;
        }
    }
}

// A task that is a whole frame is composed by its worker at once; any other is a run of a cut frame.
inline bool task_whole(const FrameTask& tk, const std::vector<int64_t>& n_rays) { return tk.r0 == 0 && tk.r1 == n_rays[tk.frame]; }

// Where the runs of cut frames go: a worker keeps the maps of the runs it renders back to back in one range buffer (20 B per ray).
struct FramePartition {
    std::vector<char> composes;         // [G] the worker composes a frame: a whole one of its own, or a cut one it owns
    std::vector<size_t> part_off;       // [tasks] a run's offset into its worker's range buffer, in rays (0 for a whole frame)
    std::vector<size_t> part_rays;      // [G] rays of a worker's range buffer
    bool split = false;                 // some frame is cut
};

inline FramePartition partition_frames(const std::vector<FrameTask>& tasks, const std::vector<int64_t>& n_rays, int G) {
    FramePartition p{std::vector<char>(G, 0), std::vector<size_t>(tasks.size(), 0), std::vector<size_t>(G, 0)};
    for (size_t t = 0; t < tasks.size(); ++t) {
        const FrameTask& tk = tasks[t];
        if (task_whole(tk, n_rays)) { p.composes[tk.worker] = 1; continue; }
        p.split = true;
        p.composes[tk.owner] = 1;
        p.part_off[t] = p.part_rays[tk.worker];
        p.part_rays[tk.worker] += (size_t)(tk.r1 - tk.r0);
    }
    return p;
}

// One frame buffer of hw pixels, on the device and in the pinned staging: rgb [hw,3] | disp [hw] | acc [hw] floats, then the uint8
// frame rgb8 [hw,3], its room rounded up to 256 bytes.  `bytes` of a region are also a frame's stride in the caller's result array.
struct FrameRegion { size_t off, bytes; };
struct FrameLayout {
    size_t hw;
    FrameRegion rgb() const { return {0, hw * 12}; }
    FrameRegion disp() const { return {hw * 12, hw * 4}; }
    FrameRegion acc() const { return {hw * 16, hw * 4}; }
    FrameRegion rgb8() const { return {hw * 20, hw * 3}; }
    size_t bytes() const { return hw * 20 + ((hw * 3 + 255) & ~size_t(255)); }
};
