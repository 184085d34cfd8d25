// pg_handle.h -- the renderer handle behind the C ABI (include/posegen_hip.h), shared by the translation units that implement
// its entry points: pg_api.hip (handle, weights, ray-level rendering), pg_frames.hip (frames), pg_train.hip (the training step),
// pg_mesh.hip, pg_poseopt.hip, pg_batch.hip, pg_metrics.hip, pg_scene.hip, pg_posescore.hip, pg_smpl.hip, pg_kploss.hip,
// pg_trainloss.hip, pg_regressor.hip, pg_disc.hip (include/posegen_gan.h), pg_gen.hip (include/posegen_generator.h), pg_hmr.hip (include/posegen_regressor.h), pg_optim.hip (include/posegen_optim.h).  Each of the last sixteen keeps its state in its slot of the handle's table (pg_modules.h):
// pg_state creates it on first use, h->mods.peek reads it, and the state's destructor frees what it owns.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "../../include/posegen_hip.h"
#include "pg_bank.h"
#include "pg_layout.h"
#include "pg_modules.h"

// A buffer that only ever grows (pg_grow / pg_grow_pinned below): on the device, or page-locked on the host (two types: neither
// is ever freed as the other).
template <bool PINNED> struct Buf {
    uint8_t* p = nullptr;
    size_t bytes = 0;
    template <typename T = uint8_t> T* as() const { return reinterpret_cast<T*>(p); }
};
using DevBuf = Buf<false>;
using PinBuf = Buf<true>;
template <bool PINNED> void pg_release(Buf<PINNED>& b) {
    if (b.p) (void)(PINNED ? hipHostFree(b.p) : hipFree(b.p));
    b = Buf<PINNED>();
}

// The handle is its active subject (pg_bank.h): net, cut, tau, emb_set and d_cut below are that model's; the other subjects of the
// bank wait in `bank` and are swapped in by pg_select_subject.
struct pg_handle : Subject {
    pg_config cfg;
    int device = 0;
    int n_cu = 256;
    int clock_khz = 0;
    char err[512] = "";
    Bank bank;                       // pg_set_subject_count / pg_select_subject
    DevBuf ws;                       // a ray-level call's workspace (pg_api.hip carve_ws)
    DevBuf fws;                      // frame front/back end: ray_batch, cams, rgb/disp/acc maps of the box (pg_frames.hip frame_ws)
    DevBuf sc_part;                  // partial nanmean sums (doubles) of the two-launch coarse sampler (pg_kernels.hip)
    DevBuf rec;                      // per-ray records of the factorised 16-bit path: Y [n + pad, 8 KiB] then (a, b) [n + pad, 768 B]
    long long rec_pad_n = -1;        // (n, Y bytes per ray) whose padding records are currently zero (-1: none)
    int rec_pad_y = 0;
    void* rec_pad_stream = nullptr;  // the stream that memset was issued on: a call on another stream zeroes again (no ordering between streams)
    // in-process multi-device rendering (pg_render_frames): the primary handle owns one sub-handle per
    // further device; every handle has a stream of its own for that path
    std::vector<pg_handle*> peers;
    hipStream_t own_stream = nullptr;
    bool far_skip = true;            // pg_set_far_skip (test / measurement aid)
    bool empty_skip = true;          // pg_set_empty_skip: waves whose points are all empty leave the colour branch out (pg_eval16r.hip)
    uint32_t* wave_counts = nullptr; // pg_debug_wave_counts: device words the counting instantiation of render launches adds to
    int onchip_mode = PG_ONCHIP_AUTO;        // pg_set_onchip (initial value: POSEGEN_ONCHIP)
    int train_precision = PG_PREC_FP32;      // pg_set_train_precision: arithmetic of the training step (fp32 like the reference, or bf16)
    bool profiling = false;
    std::vector<hipEvent_t> ev_free;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_aux;      // the record kernel in front of a factorised launch
    int64_t aux_n = 0;               // record launches / their device time already folded in by a pg_profile_read
    double aux_ms = 0.0;
    int64_t prof_points = 0;
    Modules mods;                    // the sixteen modules' states (pg_modules.h; pg_state below): each struct says beside its code what it keeps
    std::vector<float> grid_t;       // pg_grid_density: the host copy of the axis table t[R] while its upload is in flight
    bool tape_out = false;           // a pg_train_forward whose backward has not run yet: the bank stays as it is until then
};

// scratch of pg_launch_sample_coarse for n rays in chunks of `chunk` (null when the one-launch form runs)
int pg_sc_scratch(pg_handle* h, long long n, int chunk, double** out);
// the pose / cylinder stride of a ray-level call (`stage`: the stage entry points' shorter wording)
int pg_check_pose_stride(pg_handle* h, long long v, bool stage);
int pg_check_cyl_stride(pg_handle* h, long long v, bool stage);
// the joint selection of a pose call `who` (pg_pose_scores, pg_pose_loss): J_in, `joints` (null: all, and *J becomes J_in), *J against
// PG_POSE_MAX_JOINTS, the entries' range, `root`, and with `once` that no joint is named twice
constexpr int PG_POSE_MAX_JOINTS = 64;
int pg_check_joint_selection(pg_handle* h, const char* who, int J_in, const int32_t* joints, int* J, int root, bool once);
// p is not on a multiple of `a` bytes (a: the size of the element it points to)
inline bool pg_misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

// records the message (handle and thread-local "last error") and returns `code`
int pg_fail(pg_handle* h, int code, const char* fmt, ...);
// the module's state S on the handle, created on first use
template <class S> int pg_state(pg_handle* h, S*& out) {
    out = h->mods.get<S>();
    return out ? PG_OK : pg_fail(h, PG_ENOMEM, "out of memory for a module's state");
}
// `need` bytes in a buffer that only ever grows, on the current device: one that is too small is freed (after a
// hipDeviceSynchronize: what read it has to finish first; its contents are void) and allocated again with `alloc` bytes (0: need).
// A failing allocation leaves the buffer empty.  The pinned twin frees without the synchronise: its owner knows when the copies
// out of it have finished.
int pg_grow(pg_handle* h, DevBuf& b, size_t need, const char* what, size_t alloc = 0);
int pg_grow_pinned(pg_handle* h, PinBuf& b, size_t need, const char* what, size_t alloc = 0);

// A ring of pinned host / device buffer pairs for a call's small host arrays (a batch's image rows, a regressor batch's crop items).
// A slot is reused only after the copy out of its host buffer has finished (its event), so a call neither waits for the stream nor
// overwrites data still in flight.  pg_ring_upload copies `bytes` of `src` into the next slot (grown to `alloc` bytes when too small)
// and returns the slot's device buffer.
struct UploadRing {
    static constexpr int SLOTS = 8;
    struct Slot {
        PinBuf host;
        DevBuf dev;
        hipEvent_t done = nullptr;
    } slot[SLOTS];
    unsigned next = 0;
};
int pg_ring_upload(pg_handle* h, UploadRing& ring, const void* src, size_t bytes, size_t alloc, const char* what, hipStream_t st, const void** dev);
void pg_ring_release(UploadRing& ring);

// A buffer carved into arrays, each on a 256-byte boundary.  The list of take<T>(count) calls runs twice: over a Carver without a
// base, which only adds the sizes up (the pointers come out null), then over the allocation -- an array cannot be carved without
// being counted.
struct Carver {
    uint8_t* base = nullptr;
    size_t off = 0;
    template <typename T> T* take(size_t count, bool wanted = true) {
        if (!wanted) return nullptr;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

#define PG_HIP(h, call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return pg_fail(h, PG_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// a step that fails: PG_TRY hands the callee's code up (the callee has recorded its message), PG_TRY_LAUNCH records a launcher's
// hipError_t; PG_LAUNCH_CHECK is the latter behind a hipLaunchKernelGGL
#define PG_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)
#define PG_TRY_LAUNCH(h, what, call)                                                                                            \
    do { const int e_ = (int)(call); if (e_) return pg_fail(h, PG_EHIP, "%s launch failed: %s", what, hipGetErrorString((hipError_t)e_)); } while (0)
#define PG_LAUNCH_CHECK(h, what) PG_TRY_LAUNCH(h, what, hipGetLastError())
