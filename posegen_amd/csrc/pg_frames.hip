// pg_frames.hip -- the frame level of the C ABI, host side only (the kernels are pg_kernels.hip's): the frame front and back end
// (rays of a box generated, rendered and composed into the frame on the device: pg_render_frame, pg_render_frame_range,
// pg_compose_frame; the front end alone for tests: pg_stage_frame_rays) and in-process multi-device rendering of a batch of frames (pg_render_frames, pg_render_frames_subjects) over
// the plan of pg_frames_plan.h.  What a device keeps between calls of the latter is FramesState, behind the handle's `frames`.
#include <hip/hip_runtime.h>

#include <cstring>
#include <thread>

#include "pg_frames.h"
#include "pg_frames_plan.h"
#include "pg_handle.h"
#include "pg_launch.h"

// ---- frame front / back end: helpers shared by pg_render_frame (one device), pg_render_frames and pg_render_scene (pg_frames.h) ----
int frame_geom(pg_handle* h, int H, int W, const float* c2w, const float* intrinsics, const int* box, float near,
               float far, float cam, pgk::FrameGeom* g) {
    if (H <= 0 || W <= 0 || !c2w || !intrinsics || !box) return pg_fail(h, PG_EINVAL, "frame: null/non-positive argument");
    g->H = H; g->W = W;
    g->tlx = box[0] < 0 ? 0 : box[0]; g->tly = box[1] < 0 ? 0 : box[1];
    const int brx = box[2] > W ? W : box[2], bry = box[3] > H ? H : box[3];
    g->bw = brx > g->tlx ? brx - g->tlx : 0; g->bh = bry > g->tly ? bry - g->tly : 0;
    g->fx = intrinsics[0]; g->fy = intrinsics[1]; g->cx = intrinsics[2]; g->cy = intrinsics[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) g->R[3 * r + c] = c2w[4 * r + c];
        g->t[r] = c2w[4 * r + 3];
    }
    g->near = near; g->far = far; g->cam = cam;
    return PG_OK;
}

namespace {

// Frame workspace of `h`: ray_batch rows and cams of a range of n_range rays, the maps of a WHOLE box of
// n rays (n = 0: none -- the range's maps live in a buffer of the caller), coarse-pass scratch of the range.
int frame_ws(pg_handle* h, int64_t n, int64_t n_range, float** rays, float** cams, FrameMaps* maps, pg_outputs* scratch) {
    auto carve = [&](Carver& c) {
        *rays = c.take<float>((size_t)n_range * 11);
        *cams = c.take<float>((size_t)n_range);
        maps->rgb_map = c.take<float>((size_t)n * 3);
        maps->disp_map = c.take<float>((size_t)n);
        maps->acc_map = c.take<float>((size_t)n);
        scratch->rgb0 = c.take<float>((size_t)n_range * 3);
        scratch->disp0 = c.take<float>((size_t)n_range);
        scratch->acc0 = c.take<float>((size_t)n_range);
    };
    Carver sizes;
    carve(sizes);
    PG_TRY(pg_grow(h, h->fws, sizes.off, "frame workspace", sizes.off + sizes.off / 8));
    Carver c{h->fws.p};
    carve(c);
    return PG_OK;
}

}  // namespace

int frame_render_range(pg_handle* h, void* stream, const pgk::FrameGeom& g, int64_t r0, int64_t r1, const float* skts,
                       const float* cyl, int n_samples, int n_importance, int flags, FrameMaps* maps, const FrameMaps* ext,
                       const FrameLists* lists) {
    const int64_t n = (int64_t)g.bw * g.bh;
    if (r0 < 0 || r1 > n || r0 > r1) return pg_fail(h, PG_EINVAL, "frame range [%lld, %lld) outside the box of %lld rays", (long long)r0, (long long)r1, (long long)n);
    if (r0 % h->cfg.chunk != 0) return pg_fail(h, PG_EINVAL, "frame range must start on a nanmean group boundary (chunk %d)", h->cfg.chunk);
    PG_HIP(h, hipSetDevice(h->device));
    float *rays, *cams;
    pg_outputs out{};
    FrameMaps own{};
    PG_TRY(frame_ws(h, ext ? 0 : n, r1 - r0, &rays, &cams, &own, &out));
    if (maps) *maps = ext ? *ext : own;
    if (r1 == r0) return PG_OK;
    if (ext) { out.rgb_map = ext->rgb_map; out.disp_map = ext->disp_map; out.acc_map = ext->acc_map; }
    else { out.rgb_map = own.rgb_map + r0 * 3; out.disp_map = own.disp_map + r0; out.acc_map = own.acc_map + r0; }
    if (lists && n_importance > 0) { out.z_fine = lists->z; out.raw_fine = lists->raw; }
    else if (lists) { out.z_coarse = lists->z; out.raw_coarse = lists->raw; }
    const bool fc = h->cfg.framecode_ch > 0;
    PG_TRY_LAUNCH(h, "frame ray kernel", pg_launch_frame_rays(&g, r0, r1 - r0, rays, fc ? cams : nullptr, stream));
    return pg_render_rays(h, stream, r1 - r0, rays, skts, 0, cyl, 0, fc ? cams : nullptr, n_samples, n_importance, flags, &out);
}

int frame_compose(pg_handle* h, void* stream, const pgk::FrameGeom& g, const FrameMaps& maps, const float* bg, float base_bg,
                  float* rgb, float* disp, float* acc, uint8_t* rgb8) {
    PG_TRY_LAUNCH(h, "frame compose kernel", pg_launch_frame_compose(&g, maps.rgb_map, maps.disp_map, maps.acc_map, bg, base_bg, rgb, disp, acc, rgb8, stream));
    return PG_OK;
}

namespace {

// ---- pg_render_frames: per-device resources kept on the handle between calls -----------------------------------
constexpr int NBUF = 2;                 // frame buffers in rotation: frame k+1 composes while frame k copies out
constexpr size_t POSE_BYTES = (384 + 8) * sizeof(float);    // skts + cyl of one frame

struct FramesState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_FRAMES;
    ~FramesState() override {
        for (int b = 0; b < NBUF; ++b) {
            pg_release(frame[b]);
            if (copied[b]) (void)hipEventDestroy(copied[b]);
            if (composed[b]) (void)hipEventDestroy(composed[b]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (DevBuf* b : {&bg, &poses, &part}) pg_release(*b);
        pg_release(stage);
    }
    size_t hw = 0;                      // pixels the frame buffers were sized for
    DevBuf frame[NBUF];                 // FrameLayout
    hipEvent_t composed[NBUF] = {};     // buffer b holds a finished frame (render stream)
    hipEvent_t copied[NBUF] = {};       // the device-to-host copy out of buffer b has finished (copy stream)
    hipStream_t copy_stream = nullptr;
    DevBuf bg;                          // background [hw,3] (uploaded per call when given)
    DevBuf poses;                       // skts of all frames of the call [F,384], then their cyls [F,5]
    DevBuf part;                        // packed maps (20 B per ray) of the ray ranges of cut frames this device renders
    PinBuf stage;                       // pinned host staging of NBUF frames (results that land in pageable memory)
};

// the state of a device of the running call (frames_ensure has created it)
FramesState& frames_of(pg_handle* h) { return *h->mods.peek<FramesState>(); }

// grow-only: nothing is allocated or freed by a call whose sizes an earlier call has seen
int frames_ensure(pg_handle* h, size_t hw, size_t n_frames, size_t part_rays, const float* bg_host, bool staged) {
    FramesState* cp = nullptr;
    PG_TRY(pg_state(h, cp));
    FramesState& c = *cp;
    const FrameLayout lay{hw};
    PG_HIP(h, hipSetDevice(h->device));
    if (!c.copy_stream) PG_HIP(h, hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < NBUF; ++b) {
        if (!c.copied[b]) PG_HIP(h, hipEventCreateWithFlags(&c.copied[b], hipEventDisableTiming));
        if (!c.composed[b]) PG_HIP(h, hipEventCreateWithFlags(&c.composed[b], hipEventDisableTiming));
    }
    if (hw > c.hw) {
        c.hw = 0;                       // (what a failing allocation leaves behind)
        for (int b = 0; b < NBUF; ++b) PG_TRY(pg_grow(h, c.frame[b], lay.bytes(), "frame buffer"));
        c.hw = hw;
    }
    if (bg_host) {
        PG_TRY(pg_grow(h, c.bg, lay.rgb().bytes, "frame background"));
        PG_HIP(h, hipMemcpy(c.bg.p, bg_host, lay.rgb().bytes, hipMemcpyHostToDevice));
    }
    PG_TRY(pg_grow(h, c.poses, n_frames * POSE_BYTES, "frame pose buffer", (n_frames + n_frames / 2 + 8) * POSE_BYTES));
    PG_TRY(pg_grow(h, c.part, part_rays * 20, "frame range buffer", (part_rays + part_rays / 4) * 20));
    if (staged && NBUF * lay.bytes() > c.stage.bytes) {
        PG_HIP(h, hipDeviceSynchronize());
        PG_TRY(pg_grow_pinned(h, c.stage, NBUF * lay.bytes(), "frame staging"));
    }
    return PG_OK;
}

// page-locked host memory (hipHostMalloc / hipHostRegister, e.g. a torch tensor with pin_memory=True)?
bool host_pinned(const void* p) {
    if (!p) return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// Output pipeline of one worker: frame k of the worker composes into device buffer k % NBUF on the render stream
// while frame k - 1 is copied to the host on the copy stream; nothing blocks the host thread before the call's end
// (results in pageable memory go through pinned staging and are moved by the worker thread one frame later).
struct FrameOut {
    pg_handle* h;
    FramesState& c;
    hipStream_t st;
    FrameLayout lay;
    struct Result { uint8_t* host; FrameRegion r; } res[4];     // the caller's rgbs, disps, accs, rgb8 (null: not wanted)
    bool staged;
    const float* d_bg;
    float base_bg;
    int k = 0;
    int pend[NBUF];
    FrameOut(pg_handle* h_, size_t hw, float* rgbs, float* disps, float* accs, uint8_t* rgb8, bool stg, bool bg, float bb)
        : h(h_), c(frames_of(h_)), st(h_->own_stream), lay{hw},
          res{{(uint8_t*)rgbs, lay.rgb()}, {(uint8_t*)disps, lay.disp()}, {(uint8_t*)accs, lay.acc()}, {rgb8, lay.rgb8()}},
          staged(stg), d_bg(bg ? c.bg.as<float>() : nullptr), base_bg(bb) { std::fill(pend, pend + NBUF, -1); }
    uint8_t* stage(int b) const { return c.stage.p + (size_t)b * lay.bytes(); }
    int drain(int b) {              // the staged frame of buffer b -> the caller's (pageable) arrays
        const int f = pend[b];
        if (f < 0) return PG_OK;
        PG_HIP(h, hipEventSynchronize(c.copied[b]));
        for (const Result& o : res)
            if (o.host) std::memcpy(o.host + (size_t)f * o.r.bytes, stage(b) + o.r.off, o.r.bytes);
        pend[b] = -1;
        return PG_OK;
    }
    int put(int f, const pgk::FrameGeom& g, const FrameMaps& maps) {
        const int b = k++ % NBUF;
        if (staged) PG_TRY(drain(b));
        PG_HIP(h, hipStreamWaitEvent(st, c.copied[b], 0));          // buffer b's previous copy-out (no-op before the first)
        uint8_t* base = c.frame[b].p;
        auto at = [&](FrameRegion r) { return reinterpret_cast<float*>(base + r.off); };
        PG_TRY(frame_compose(h, st, g, maps, d_bg, base_bg, at(lay.rgb()), at(lay.disp()), at(lay.acc()), res[3].host ? base + lay.rgb8().off : nullptr));
        PG_HIP(h, hipEventRecord(c.composed[b], st));
        PG_HIP(h, hipStreamWaitEvent(c.copy_stream, c.composed[b], 0));
        for (const Result& o : res)
            if (o.host) PG_HIP(h, hipMemcpyAsync(staged ? stage(b) + o.r.off : o.host + (size_t)f * o.r.bytes, base + o.r.off, o.r.bytes, hipMemcpyDeviceToHost, c.copy_stream));
        PG_HIP(h, hipEventRecord(c.copied[b], c.copy_stream));
        if (staged) pend[b] = f;
        return PG_OK;
    }
    int finish() {
        for (int b = 0; staged && b < NBUF; ++b) PG_TRY(drain(b));
        PG_HIP(h, hipStreamSynchronize(c.copy_stream));
        return PG_OK;
    }
};

// One pg_render_frames call: its arguments, its plan, and one worker per device (worker 0 on the calling thread).
struct FramesCall {
    int n_frames;
    const float *skts, *cyls;
    int n_samples, n_importance, flags;
    const int32_t* subjects;
    std::vector<pg_handle*> wk;             // [G] the handles: the primary, then its peers
    std::vector<pgk::FrameGeom> geo;        // [F]
    std::vector<int64_t> nr;                // [F] rays of the frames' boxes
    std::vector<FrameTask> tasks;
    FramePartition part;
    std::vector<int> rc;                    // [G] a worker's first failure (its message is on its handle)
    std::vector<FrameMaps> maps_of;         // [tasks] where phase A left the task's maps
    std::vector<FrameOut> outs;             // [G]

    bool check(int k, hipError_t e, const char* what) {
        if (e != hipSuccess && rc[k] == PG_OK) rc[k] = pg_fail(wk[k], PG_EHIP, "%s failed on device %d: %s", what, wk[k]->device, hipGetErrorString(e));
        return e == hipSuccess;
    }
    // phase A: every worker renders its tasks; whole frames are composed and handed to the output pipeline at once,
    // the runs of cut frames stay in the worker's range buffer for the owner
    void phase_a(int k) {
        pg_handle* hh = wk[k];
        if (!check(k, hipSetDevice(hh->device), "hipSetDevice")) return;
        hipStream_t st = hh->own_stream;
        FramesState& c = frames_of(hh);
        float* d_skts = c.poses.as<float>();
        float* d_cyls = d_skts + (size_t)n_frames * 384;
        // (pageable sources: the runtime stages them before the calls return; the kernels are ordered behind on `st`)
        if (!check(k, hipMemcpyAsync(d_skts, skts, (size_t)n_frames * 384 * sizeof(float), hipMemcpyHostToDevice, st), "pose upload")) return;
        if (!check(k, hipMemcpyAsync(d_cyls, cyls, (size_t)n_frames * 5 * sizeof(float), hipMemcpyHostToDevice, st), "cylinder upload")) return;
        for (size_t t = 0; t < tasks.size() && rc[k] == PG_OK; ++t) {
            const FrameTask& tk = tasks[t];
            if (tk.worker != k) continue;
            const int f = tk.frame;
            // this device's own selection (each worker thread touches its own handle only): a pointer swap between two enqueues
            if (subjects) bank_select(*hh, hh->bank, subjects[f]);
            const float *sk = d_skts + (size_t)f * 384, *cy = d_cyls + (size_t)f * 5;
            if (task_whole(tk, nr)) {
                rc[k] = frame_render_range(hh, st, geo[f], tk.r0, tk.r1, sk, cy, n_samples, n_importance, flags, &maps_of[t]);
                if (rc[k]) return;
                rc[k] = outs[k].put(f, geo[f], maps_of[t]);
            } else {
                const size_t n = (size_t)(tk.r1 - tk.r0);
                if (n == 0) continue;
                float* p = c.part.as<float>() + part.part_off[t] * 5;
                const FrameMaps ext{p, p + n * 3, p + n * 4};
                rc[k] = frame_render_range(hh, st, geo[f], tk.r0, tk.r1, sk, cy, n_samples, n_importance, flags, &maps_of[t], &ext);
            }
        }
        if (rc[k] == PG_OK) check(k, hipStreamSynchronize(st), "hipStreamSynchronize");      // phase B reads other workers' range buffers
    }
    // phase B: the owner of a cut frame gathers all its runs (device to device), composes, copies out
    void phase_b(int k) {
        pg_handle* hh = wk[k];
        if (!check(k, hipSetDevice(hh->device), "hipSetDevice")) return;
        hipStream_t st = hh->own_stream;
        for (int f = 0; f < n_frames && rc[k] == PG_OK; ++f) {
            bool mine = false;
            for (const FrameTask& tk : tasks) mine = mine || (tk.frame == f && tk.owner == k && !task_whole(tk, nr));
            if (!mine) continue;
            float *rays, *cams_d;
            FrameMaps box{};
            pg_outputs scratch{};
            rc[k] = frame_ws(hh, nr[f], 0, &rays, &cams_d, &box, &scratch);     // phase A is over: the workspace is free
            if (rc[k]) return;
            for (size_t u = 0; u < tasks.size(); ++u) {
                const FrameTask& pt = tasks[u];
                if (pt.frame != f || pt.r1 == pt.r0) continue;
                const int src_dev = wk[pt.worker]->device;
                const size_t n = (size_t)(pt.r1 - pt.r0);
                if (!check(k, hipMemcpyPeerAsync(box.rgb_map + pt.r0 * 3, hh->device, maps_of[u].rgb_map, src_dev, n * 12, st), "peer copy") ||
                    !check(k, hipMemcpyPeerAsync(box.disp_map + pt.r0, hh->device, maps_of[u].disp_map, src_dev, n * 4, st), "peer copy") ||
                    !check(k, hipMemcpyPeerAsync(box.acc_map + pt.r0, hh->device, maps_of[u].acc_map, src_dev, n * 4, st), "peer copy")) return;
            }
            rc[k] = outs[k].put(f, geo[f], box);
        }
    }
    void finish(int k) {
        if (rc[k] != PG_OK || !part.composes[k]) return;
        if (!check(k, hipSetDevice(wk[k]->device), "hipSetDevice")) return;
        rc[k] = outs[k].finish();
    }
    void run(void (FramesCall::*fn)(int)) {
        std::vector<std::thread> th;
        for (int k = 1; k < (int)wk.size(); ++k) th.emplace_back(fn, this, k);
        (this->*fn)(0);
        for (auto& t : th) t.join();
    }
};

}  // namespace

extern "C" {

int pg_render_frame(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics,
                    const int* box, float near, float far, const float* skts, const float* cyl, float cam,
                    int n_samples, int n_importance, int flags, const float* bg, float base_bg,
                    float* rgb, float* disp, float* acc, uint8_t* rgb8) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!skts || !cyl || !rgb) return pg_fail(h, PG_EINVAL, "pg_render_frame: null argument");
    pgk::FrameGeom g{};
    PG_TRY(frame_geom(h, H, W, c2w, intrinsics, box, near, far, cam, &g));
    FrameMaps maps{};
    PG_TRY(frame_render_range(h, stream, g, 0, (int64_t)g.bw * g.bh, skts, cyl, n_samples, n_importance, flags, &maps));
    return frame_compose(h, stream, g, maps, bg, base_bg, rgb, disp, acc, rgb8);
}

int pg_render_frame_range(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics,
                          const int* box, float near, float far, const float* skts, const float* cyl, float cam,
                          int n_samples, int n_importance, int flags, int64_t ray_begin, int64_t ray_end,
                          float* rgb_map, float* disp_map, float* acc_map) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!skts || !cyl || !rgb_map || !disp_map || !acc_map) return pg_fail(h, PG_EINVAL, "pg_render_frame_range: null argument");
    pgk::FrameGeom g{};
    PG_TRY(frame_geom(h, H, W, c2w, intrinsics, box, near, far, cam, &g));
    const FrameMaps ext{rgb_map, disp_map, acc_map};
    return frame_render_range(h, stream, g, ray_begin, ray_end, skts, cyl, n_samples, n_importance, flags, nullptr, &ext);
}

int pg_compose_frame(pg_handle* h, void* stream, int H, int W, const int* box, const float* rgb_map, const float* disp_map,
                     const float* acc_map, const float* bg, float base_bg, float* rgb, float* disp, float* acc, uint8_t* rgb8) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (H <= 0 || W <= 0 || !box || !rgb) return pg_fail(h, PG_EINVAL, "pg_compose_frame: null/non-positive argument");
    pgk::FrameGeom g{};
    const float c2w[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, intr[4] = {1.f, 1.f, 0.f, 0.f};
    PG_TRY(frame_geom(h, H, W, c2w, intr, box, 0.f, 1.f, -1.f, &g));
    if ((int64_t)g.bw * g.bh > 0 && (!rgb_map || !disp_map || !acc_map)) return pg_fail(h, PG_EINVAL, "pg_compose_frame: null map of a non-empty box");
    PG_HIP(h, hipSetDevice(h->device));
    const FrameMaps maps{const_cast<float*>(rgb_map), const_cast<float*>(disp_map), const_cast<float*>(acc_map)};
    return frame_compose(h, stream, g, maps, bg, base_bg, rgb, disp, acc, rgb8);
}

int pg_stage_frame_rays(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics, const int* box,
                        float near, float far, float cam, int64_t ray_begin, int64_t ray_end, float* rays, float* cams) {
    // the host arguments first (pg_fail takes a null handle): what is refused does not depend on there being a device
    if (!rays) return pg_fail(h, PG_EINVAL, "pg_stage_frame_rays: null argument");
    pgk::FrameGeom g{};
    PG_TRY(frame_geom(h, H, W, c2w, intrinsics, box, near, far, cam, &g));
    const int64_t n = (int64_t)g.bw * g.bh;
    if (ray_begin < 0 || ray_end > n || ray_begin > ray_end)
        return pg_fail(h, PG_EINVAL, "frame range [%lld, %lld) outside the box of %lld rays", (long long)ray_begin, (long long)ray_end, (long long)n);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY_LAUNCH(h, "frame ray kernel", pg_launch_frame_rays(&g, ray_begin, ray_end - ray_begin, rays, cams, stream));
    return PG_OK;
}

int pg_plan_frames(int n_frames, const int64_t* n_rays, int n_workers, int chunk, int32_t* out_tasks /*[cap,5]*/, int cap, int* n_tasks) {
    if (n_frames < 0 || !n_rays || n_workers < 1 || chunk < 1 || !n_tasks) return pg_fail(nullptr, PG_EINVAL, "pg_plan_frames: bad argument");
    std::vector<FrameTask> t;
    plan_frames(std::vector<int64_t>(n_rays, n_rays + n_frames), n_workers, chunk, &t);
    *n_tasks = (int)t.size();
    if (out_tasks) {
        if ((int)t.size() > cap) return pg_fail(nullptr, PG_EINVAL, "pg_plan_frames: %zu tasks exceed the capacity %d", t.size(), cap);
        for (size_t i = 0; i < t.size(); ++i) {
            out_tasks[5 * i] = t[i].frame; out_tasks[5 * i + 1] = (int32_t)t[i].r0; out_tasks[5 * i + 2] = (int32_t)t[i].r1;
            out_tasks[5 * i + 3] = t[i].worker; out_tasks[5 * i + 4] = t[i].owner;
        }
    }
    return PG_OK;
}

int pg_render_frames(pg_handle* h, int n_frames, int H, int W, const float* c2ws, const float* intrinsics, const int* boxes,
                     float near, float far, const float* skts, const float* cyls, const float* cams, int n_samples,
                     int n_importance, int flags, const float* bg, float base_bg, float* rgbs, float* disps, float* accs,
                     uint8_t* rgb8) {
    return pg_render_frames_subjects(h, n_frames, H, W, c2ws, intrinsics, boxes, near, far, skts, cyls, cams, n_samples, n_importance,
                                     flags, bg, base_bg, rgbs, disps, accs, rgb8, nullptr);
}

int pg_render_frames_subjects(pg_handle* h, int n_frames, int H, int W, const float* c2ws, const float* intrinsics, const int* boxes,
                              float near, float far, const float* skts, const float* cyls, const float* cams, int n_samples,
                              int n_importance, int flags, const float* bg, float base_bg, float* rgbs, float* disps, float* accs,
                              uint8_t* rgb8, const int32_t* subjects) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_frames < 0 || H <= 0 || W <= 0 || !c2ws || !intrinsics || !boxes || !skts || !cyls || (!rgbs && !rgb8))
        return pg_fail(h, PG_EINVAL, "pg_render_frames: null/negative argument");
    if (n_frames == 0) return PG_OK;
    if (subjects) {
        if (h->tape_out) return pg_fail(h, PG_EINVAL, "pg_render_frames_subjects: a training tape is outstanding (run its backward first)");
        for (int f = 0; f < n_frames; ++f)
            if (subjects[f] < 0 || subjects[f] >= bank_count(h->bank))
                return pg_fail(h, PG_EINVAL, "pg_render_frames_subjects: frame %d names subject %d of %d", f, subjects[f], bank_count(h->bank));
    }
    const int active0 = h->bank.active;         // (every device's: pg_select_subject reaches them all)
    // Worker 0 runs on the primary handle's own stream over the primary's workspaces: everything the caller
    // queued on ITS stream (pg_render_rays / pg_render_frame are asynchronous and use the same buffers) must
    // have finished first.  The call is synchronous anyway.
    PG_HIP(h, hipSetDevice(h->device));
    PG_HIP(h, hipDeviceSynchronize());
    FramesCall call{n_frames, skts, cyls, n_samples, n_importance, flags, subjects, {h}};
    call.wk.insert(call.wk.end(), h->peers.begin(), h->peers.end());
    const std::vector<pg_handle*>& wk = call.wk;
    const int G = (int)wk.size();
    const size_t hw = (size_t)H * W;
    call.geo.resize(n_frames);
    call.nr.resize(n_frames);
    for (int f = 0; f < n_frames; ++f) {
        PG_TRY(frame_geom(h, H, W, c2ws + 12 * f, intrinsics + 4 * f, boxes + 4 * f, near, far, cams ? cams[f] : -1.0f, &call.geo[f]));
        call.nr[f] = (int64_t)call.geo[f].bw * call.geo[f].bh;
    }
    plan_frames(call.nr, G, h->cfg.chunk, &call.tasks);
    call.part = partition_frames(call.tasks, call.nr, G);
    const FramePartition& part = call.part;
    // Everything a worker needs is set up BEFORE its first launch and kept on its handle between calls (no allocation
    // in a call whose sizes have been seen): the poses of all frames (one upload), two frame buffers in rotation, the
    // background, one buffer for the packed maps of the cut-frame ranges it renders, pinned staging when the
    // caller's result arrays are pageable.
    const bool staged = !(host_pinned(rgbs) && host_pinned(disps) && host_pinned(accs) && host_pinned(rgb8));
    for (int k = 0; k < G; ++k) {
        const int rc = frames_ensure(wk[k], part.composes[k] ? hw : 0, n_frames, part.part_rays[k], part.composes[k] ? bg : nullptr, staged && part.composes[k]);
        if (rc) { (void)hipSetDevice(h->device); return wk[k] == h ? rc : pg_fail(h, rc, "device %d: %s", wk[k]->device, wk[k]->err); }
    }
    call.rc.assign(G, PG_OK);
    call.maps_of.resize(call.tasks.size());
    call.outs.reserve(G);
    for (int k = 0; k < G; ++k) call.outs.emplace_back(wk[k], hw, rgbs, disps, accs, rgb8, staged, bg != nullptr, base_bg);
    call.run(&FramesCall::phase_a);
    if (part.split && std::count(call.rc.begin(), call.rc.end(), PG_OK) == G) call.run(&FramesCall::phase_b);
    call.run(&FramesCall::finish);
    if (subjects)
        for (pg_handle* w : wk) bank_select(*w, w->bank, active0);
    int rc = PG_OK;
    for (int k = 0; k < G; ++k) {
        if (call.rc[k] == PG_OK) continue;  // nothing of a failed call may still be in flight when the caller's arrays go away
        (void)hipSetDevice(wk[k]->device);
        (void)hipDeviceSynchronize();
        if (rc == PG_OK) rc = (wk[k] == h) ? call.rc[k] : pg_fail(h, call.rc[k], "device %d: %s", wk[k]->device, wk[k]->err);
    }
    (void)hipSetDevice(h->device);
    return rc;
}

}  // extern "C"
