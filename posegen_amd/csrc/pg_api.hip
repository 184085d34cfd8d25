// pg_api.hip -- C ABI of libposegen_hip.so (include/posegen_hip.h): handle, weight
// packing / upload, workspace, and the launch sequence of one render_rays call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "../../include/posegen_hip.h"
#include "pg_device.h"
#include "pg_handle.h"
#include "pg_kin.h"
#include "pg_launch.h"
#include "pg_pack.h"

namespace {

using namespace pgl;

thread_local char g_last_error[512] = "";      // pg_last_error(NULL): per host thread

}  // namespace

int pg_fail(pg_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::snprintf(g_last_error, sizeof g_last_error, "%s", buf);
    if (h) std::snprintf(h->err, sizeof h->err, "%s", buf);
    return code;
}

int pg_grow(pg_handle* h, DevBuf& b, size_t need, const char* what, size_t alloc) {
    if (need <= b.bytes) return PG_OK;
    if (b.p) { PG_HIP(h, hipDeviceSynchronize()); PG_HIP(h, hipFree(b.p)); b = DevBuf(); }
    if (alloc < need) alloc = need;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b.p), alloc);
    if (e != hipSuccess) { b = DevBuf(); return pg_fail(h, PG_ENOMEM, "%s of %zu bytes failed: %s", what, alloc, hipGetErrorString(e)); }
    b.bytes = alloc;
    return PG_OK;
}

int pg_grow_pinned(pg_handle* h, PinBuf& b, size_t need, const char* what, size_t alloc) {
    if (need <= b.bytes) return PG_OK;
    if (b.p) { PG_HIP(h, hipHostFree(b.p)); b = PinBuf(); }
    if (alloc < need) alloc = need;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&b.p), alloc, hipHostMallocDefault);
    if (e != hipSuccess) { b = PinBuf(); return pg_fail(h, PG_ENOMEM, "%s of %zu pinned bytes failed: %s", what, alloc, hipGetErrorString(e)); }
    b.bytes = alloc;
    return PG_OK;
}

int pg_ring_upload(pg_handle* h, UploadRing& ring, const void* src, size_t bytes, size_t alloc, const char* what, hipStream_t st, const void** dev) {
    UploadRing::Slot& sl = ring.slot[ring.next++ % UploadRing::SLOTS];
    if (!sl.done) PG_HIP(h, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    else PG_HIP(h, hipEventSynchronize(sl.done));
    PG_TRY(pg_grow_pinned(h, sl.host, bytes, what, alloc));
    PG_TRY(pg_grow(h, sl.dev, sl.host.bytes, what));
    std::memcpy(sl.host.p, src, bytes);
    PG_HIP(h, hipMemcpyAsync(sl.dev.p, sl.host.p, bytes, hipMemcpyHostToDevice, st));
    PG_HIP(h, hipEventRecord(sl.done, st));
    *dev = sl.dev.p;
    return PG_OK;
}

void pg_ring_release(UploadRing& ring) {
    for (auto& sl : ring.slot) {
        if (sl.done) (void)hipEventDestroy(sl.done);
        pg_release(sl.host);
        pg_release(sl.dev);
    }
    ring = UploadRing();
}

namespace {

// state setters are forwarded to the sub-handles of a multi-device handle (message of a failing one is kept)
#define PG_FORWARD(h, call)                                                                  \
    do {                                                                                     \
        for (pg_handle* sub_ : (h)->peers) {                                                 \
            pg_handle* hh = sub_;                                                            \
            const int rc_ = (call);                                                          \
            if (rc_) return pg_fail(h, rc_, "device %d: %s", hh->device, hh->err);              \
        }                                                                                    \
    } while (0)

bool is_shape_a(int prec) { return prec == PG_PREC_BF16 || prec == PG_PREC_FP16; }

// bf16x3 (every product as hi*hi + hi*lo + lo*hi of bf16 halves) is the 1e-4-grade mode at MFMA
// speed.  fp16x3 stays EXPERIMENTAL: the low half of a small value underflows fp16's exponent
// range, so it is no better than plain fp16 there (DESIGN.md "Known issues"); opt-in only.
bool x3_allowed() {
    const char* e = std::getenv("POSEGEN_EXPERIMENTAL_X3");
    return e && e[0] == '1';
}
bool is_x3(int prec) { return prec == PG_PREC_FP16X3; }

pgpack::NetTensors tensors_of(const NetState& ns, const pg_config& cfg) {
    pgpack::NetTensors t;
    for (int l = 0; l < DEPTH; ++l) {
        t.lw[l] = ns.host[2 * l].data();
        t.lb[l] = ns.host[2 * l + 1].data();
        t.lcols[l] = l == 0 ? CH_X : (l == SKIP + 1 ? CH_X + W : W);
    }
    t.alpha_w = ns.host[16].data(); t.alpha_b = ns.host[17].data();
    t.feat_w = ns.host[18].data();  t.feat_b = ns.host[19].data();
    t.view_w = ns.host[20].data();  t.view_b = ns.host[21].data();
    t.view_cols = W + CH_D + cfg.framecode_ch;
    t.rgb_w = ns.host[22].data();   t.rgb_b = ns.host[23].data();
    if (ns.fold_w.empty()) { t.fold(); ns.fold_w = t.viewf_w; ns.fold_b = t.viewf_b; }      // (every packer of the net shares it)
    else { t.viewf_w = ns.fold_w; t.viewf_b = ns.fold_b; }
    return t;
}

// multires_views = 0 (cutoff_embedder.py:20-31, 199-213 with no frequency bands): the view input is v * w, 72 channels,
// which is row 0 of the 4-band embedding (channel row*72 + 3j + c).  Its view weight [128, 256+72(+fc)] becomes the
// [128, 256+648(+fc)] matrix with the sin/cos columns zero: a zero weight adds exact zeros in every precision (and splits
// to zeros in the bf16x3 / fp16c forms), so no kernel changes.
constexpr int CH_D0 = J * 3;
void widen_view_w(const float* src, int fc, float* dst) {
    const int sc = W + CH_D0 + fc, dc = W + CH_D + fc;
    for (int o = 0; o < VW; ++o) {
        const float* r = src + (size_t)o * sc;
        float* d = dst + (size_t)o * dc;
        std::memcpy(d, r, (size_t)(W + CH_D0) * sizeof(float));
        std::memset(d + W + CH_D0, 0, (size_t)(CH_D - CH_D0) * sizeof(float));
        std::memcpy(d + W + CH_D, r + W + CH_D0, (size_t)fc * sizeof(float));
    }
}

// host copies of one net's 24 tensors (the debug packers): a [128, 256+72(+fc)] view weight is widened as the load does
void host_copy(NetState& ns, const float* const* tensors, const int64_t* shapes, int fc) {
    ns.host.assign(24, {});
    for (int i = 0; i < 24; ++i) {
        if (i == 20 && shapes[2 * i + 1] == W + CH_D0 + fc) {
            ns.host[i].resize((size_t)VW * (W + CH_D + fc));
            widen_view_w(tensors[i], fc, ns.host[i].data());
        } else ns.host[i].assign(tensors[i], tensors[i] + shapes[2 * i] * shapes[2 * i + 1]);
    }
}

// ---- which form of the fused kernel a call runs (pick_form), and what each form reads (FORMS) ---------------------------
enum Form {
    F_DIRECT16,         // pg_eval16.hip: bf16 / fp16, 32x32x16 MFMAs, direct view layer
    F_REC16,            // pg_eval16r.hip: bf16 / fp16, 16x16x32 MFMAs, the view layer factorised over per-ray records (pg_rayrec.hip)
    F_ONCHIP16,         // ... its on-chip variant: no per-ray records
    F_C2,               // pg_evalc2.hip: compensated fp16, the out tiles split over the waves
    F_KMAJOR,           // pg_eval32.hip, k-major: fp32, the split-operand precisions, and PG_PREC_FP16C where pg_evalc2.hip does not run
    F_COUNT
};

// The process's switches (A/B, debugging), read once; "0" turns a form off
// Rotation of the pass walk per round (pg_device.h PassWalk), in passes.  Odd, and 99 / 256, 99 / 128 and 35 / 64 (what is left of it
// on frames whose rows are 256, 128 or 64 passes) all have small partial quotients: the strips a workgroup visits in the few dozen
// rounds of a frame are spread evenly over the row, not clustered.
constexpr int PASS_WALK_RHO = 99;
struct Switches {
    bool view_fact = true;          // POSEGEN_VIEW_FACT=0: the direct 32x32x16 kernel (pg_eval16.hip) for every 16-bit call
    bool comp_kernel = true;        // POSEGEN_COMP_KERNEL=0: PG_PREC_FP16C in the k-major kernel of pg_eval32.hip instead of pg_evalc2.hip, same arithmetic
    int onchip = PG_ONCHIP_AUTO;    // POSEGEN_ONCHIP = 0 / 1 / 2: the pg_set_onchip mode a new handle starts in
    bool empty_skip = true;         // POSEGEN_EMPTY_SKIP=0: the pg_set_empty_skip setting a new handle starts in (A/B on one library)
    int pass_walk = PASS_WALK_RHO;  // POSEGEN_PASS_WALK=0: the static pass walk of the kernels with limb masks (pg_device.h PassWalk); n > 0: rotation n
};
const Switches& switches() {
    static const Switches sw = [] {
        auto off = [](const char* name) { const char* e = std::getenv(name); return e && e[0] == '0'; };
        Switches s;
        s.view_fact = !off("POSEGEN_VIEW_FACT");
        s.comp_kernel = !off("POSEGEN_COMP_KERNEL");
        s.empty_skip = !off("POSEGEN_EMPTY_SKIP");
        const char* e = std::getenv("POSEGEN_ONCHIP");
        s.onchip = e && e[0] == '0' ? PG_ONCHIP_RECORDS : e && e[0] == '2' ? PG_ONCHIP_ALWAYS : PG_ONCHIP_AUTO;
        if (const char* w = std::getenv("POSEGEN_PASS_WALK")) s.pass_walk = std::max(0, std::atoi(w));
        return s;
    }();
    return sw;
}

// what pick_form looks at
struct CallFacts {
    int prec;                       // kernel arithmetic of the pass (pass_precision)
    int S;                          // samples per ray
    long long pose_stride;          // 0: one pose per launch
    bool fc;                        // the config has frame codes
    bool points, pnoise;            // explicit points / position noise
    bool dbg; int dbg_stage;        // debug buffer given, and what it asks for
    int onchip_mode;                // pg_set_onchip
};

// PG_PREC_FP16M: the coarse pass of a hierarchical render only places the importance samples (and fills
// rgb0/acc0): plain fp16 there, compensated fp16 wherever the pass produces the returned maps
int pass_precision(int mode, bool guide_pass) { return mode == PG_PREC_FP16M ? (guide_pass ? PG_PREC_FP16 : PG_PREC_FP16C) : mode; }

// The on-chip variant of the 16x16x32 kernel runs for rays of at most ONCHIP_MAX_S samples, per-ray poses and frame codes included.
// The on-chip variant forms a ray's rows in every pass the ray has points in, the record variant once
// per ray in a kernel in front: measured on one box (profiles/r5_ab_onchip_by_samples.txt, bf16 512 x 512 frames) the two
// tie at 64 + 16 samples (31.7 / 31.8 ms), on-chip wins at 96 + 16 (43.3 / 43.6) and records win from 128 + 16 on (59.3 /
// 58.0; with frame codes 59.7 / 58.2) -- at a cost of 8.75 KiB of HBM per ray.  pg_set_onchip (initial value: POSEGEN_ONCHIP = 0 / 1 / 2)
// forces the record variants (0) or the on-chip ones whatever the sample count (2).
constexpr int ONCHIP_MAX_S = 112;

// The one place that decides the form.  Pure: exercised over the whole product of its facts on the host.
Form pick_form(const CallFacts& c, const Switches& sw) {
    // explicit points and position noise need q = R p + t per point: the direct kernels (no per-ray a + z b table)
    const bool from_rays = !c.points && !c.pnoise;
    if (is_shape_a(c.prec)) {
        // the 16-bit precisions factorise the view layer over rays when a pass cannot touch more than MAXR_F rays (pg_layout.h)
        if (!(from_rays && sw.view_fact && c.S >= FACT_MIN_S)) return F_DIRECT16;
        const bool by_mode = c.onchip_mode == PG_ONCHIP_ALWAYS || (c.onchip_mode == PG_ONCHIP_AUTO && c.S <= ONCHIP_MAX_S);
        // (97: the on-chip variant's limb-mask counters; 99: the stamps of a PG_STAMPS build, whichever form the mode picks)
        const bool dbg_ok = !c.dbg || c.dbg_stage == 99 || (c.dbg_stage == 97 && c.pose_stride == 0 && !c.fc);
        return by_mode && dbg_ok ? F_ONCHIP16 : F_REC16;
    }
    // PG_PREC_FP16C runs in pg_evalc2.hip (out tiles over the waves) when the points come from rays of >= pgp::T::MIN_S samples (then a
    // 128-point pass touches <= pgp::T::MAXR rays), whatever the pose stride, with or without frame codes; that kernel has no activation
    // tap (97: its limb-mask counters; 99: the stamps of a PG_STAMPS build).  Every other call, of this precision too, runs in the
    // k-major kernel of pg_eval32.hip, same arithmetic
    const bool c2 = c.prec == PG_PREC_FP16C && sw.comp_kernel && from_rays && c.S >= pgp::T::MIN_S && (!c.dbg || c.dbg_stage == 97 || c.dbg_stage == 99);
    return c2 ? F_C2 : F_KMAJOR;
}

// the usual call of a precision: rays with >= 64 samples, one pose per launch, no points, no noise, no debug.  Its form is what
// pg_load_weights packs ahead of the first render (ensure_mode_streams) and what pg_query reports
Form usual_form(const pg_handle* h, int prec) {
    return pick_form(CallFacts{prec, FACT_MIN_S, 0, h->cfg.framecode_ch > 0, false, false, false, 0, h->onchip_mode}, switches());
}

int one_wg_per_cu(void) { return 1; }

struct FormInfo {
    int stream;                     // image the kernel streams (a per-precision kind: image_of adds the pass's precision)
    int wy;                         // Y-stage weights of the record kernel in front, or the Yc table (IMG_YCODE: with frame codes only)
    int bias;                       // IMG_BIAS or IMG_BIAS16
    int rec_y_bytes;                // per-ray records: bytes of Y per ray (0: no record kernel)
    int (*points_per_pass)(void);
    int (*wgs_per_cu)(void);
    // pg_query: weight bytes a pass reads; MFMAs per 32-point group in 32x32x16 equivalents (32 768 FLOP each)
    int64_t (*stream_bytes)(int prec);
    int64_t (*mfma_per_group)(int prec, bool fc);
};
// the fp32 / split kernels keep feature_linear and the direct view layer (13 + 4 out tiles)
constexpr int64_t mfma_direct(bool fc) { return pgp::A::MFMA_PER_GROUP(fc) + (NT + 1 + NTV - (NTV + 1)) * pgp::A::HU; }
#define PG_CHUNKS(n) [](int) -> int64_t { return (int64_t)(n) * CHUNK_BYTES; }
#define PG_MFMA(expr) [](int prec, bool fc) -> int64_t { (void)prec; (void)fc; return (expr); }
constexpr FormInfo FORMS[F_COUNT] = {
    /* F_DIRECT16    */ {IMG_DIRECT, IMG_NONE, IMG_BIAS, 0, pg_eval16_points_per_pass, pg_eval16_wgs_per_cu,
                         PG_CHUNKS(pgp::A::NCHUNK), PG_MFMA(pgp::A::MFMA_PER_GROUP(fc))},
    /* F_REC16       */ {IMG_REC16, IMG_VY16, IMG_BIAS16, REC_Y_BYTES, pg_eval16_points_per_pass, pg_eval16_wgs_per_cu,
                         PG_CHUNKS(pgp::R::NCHUNK), PG_MFMA(pgp::R::MFMA16_PER_GROUP / 2)},
    /* F_ONCHIP16    */ {IMG_ONCHIP16, IMG_YCODE, IMG_BIAS16, 0, pg_eval16_points_per_pass, pg_eval16_wgs_per_cu,
                         PG_CHUNKS(pgp::R::NCHUNK_OC), PG_MFMA(pgp::R::MFMA16_PER_GROUP / 2)},
    /* F_C2 (no stream: the whole image) */
                        {IMG_C2, IMG_NONE, IMG_BIAS16, 0, pg_evalc2_points_per_pass, one_wg_per_cu,
                         [](int) -> int64_t { return pgp::T::TOTAL; }, PG_MFMA(pgp::T::MFMA16_PER_PASS / 2 / (pgp::T::PTS / 32))},
    /* F_KMAJOR      */ {IMG_DIRECT, IMG_NONE, IMG_BIAS, 0, pg_eval32_points_per_pass, one_wg_per_cu,
                         [](int prec) -> int64_t { return (int64_t)(prec == PG_PREC_FP32 ? pgp::B::NCHUNK : pgp::B::NCHUNK_FOLD) * CHUNK_BYTES; },
                         PG_MFMA(prec == PG_PREC_FP32 ? mfma_direct(fc) * 8 : (mfma_direct(fc) - NT * pgp::A::HU) * (prec == PG_PREC_FP16C ? 2 : 3))},
};
#undef PG_CHUNKS
#undef PG_MFMA
constexpr int image_of(int image, int prec) { return image >= 0 && image < IMG_PER_PREC_END ? image + prec : image; }

int ensure_rec(pg_handle* h, int64_t n, int y_bytes) {
    const size_t need = (size_t)(n + REC_PAD_RAYS) * ((size_t)y_bytes + REC_AB_BYTES);
    if (need <= h->rec.bytes) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    h->rec_pad_n = -1;
    return pg_grow(h, h->rec, need, "ray record buffer", need + need / 16);
}

// ---- the packed weight images of a net (NetState::img) ------------------------------------------------------------
struct Packed {
    std::vector<uint8_t> b;
    std::vector<float> f;           // (the fp32 tables)
    const void* data() const { return f.empty() ? static_cast<const void*>(b.data()) : f.data(); }
    size_t bytes() const { return f.empty() ? b.size() : f.size() * sizeof(float); }
};

// Image `id` of net `which`, packed from the tensors `t`; `src`: its source map as well (the images of REFORMED)
int pack_image(pg_handle* h, int which, const pgpack::NetTensors& t, int id, Packed& p, std::vector<int32_t>* src = nullptr) {
    const NetState& ns = h->net[which];
    const bool fc = h->cfg.framecode_ch > 0;
    const int prec = id < IMG_PER_PREC_END ? id % PG_PREC_COUNT : PG_PREC_FP16C;
    int rc = 0;
    switch (id < IMG_PER_PREC_END ? id - prec : id) {
    case IMG_DIRECT:
        if ((rc = pgpack::pack_stream(t, prec, fc, p.b))) return pg_fail(h, PG_EINVAL, "weight stream packing failed (%d) for precision %d", rc, prec);
        break;
    case IMG_REC16:
        if ((rc = pgpack::pack_stream_r(t, prec, p.b))) return pg_fail(h, PG_EINVAL, "16x16x32 weight stream packing failed (%d) for precision %d", rc, prec);
        break;
    case IMG_ONCHIP16:
        if ((rc = pgpack::pack_stream_r(t, prec, p.b, true, src))) return pg_fail(h, PG_EINVAL, "on-chip 16x16x32 weight stream packing failed (%d) for precision %d", rc, prec);
        break;
    case IMG_VY16:
        if (pgpack::pack_vy(t, prec, fc, p.b) != 0) return pg_fail(h, PG_EINVAL, "Y-stage weight packing failed for precision %d", prec);
        break;
    case IMG_C2:
        if ((rc = pgpack::pack_c2(t, fc, p.b, src))) return pg_fail(h, PG_EINVAL, "compensated-fp16 tile-split weight packing failed (%d)", rc);
        break;
    case IMG_YCODE: {
        // The frame code's part of the view layer for every code (and the mean row, embedding.py:25-26), as the on-chip variant reads it:
        // Yc[c][o] = sum_k W_view[o][256 + 648 + k] codes[c][k] in fp32 (sums in double) -- 16 products per value once per
        // pg_set_framecodes / pg_load_weights instead of once per ray.
        if (ns.codes_host.empty()) return pg_fail(h, PG_ESTATE, "frame codes of net %d not set (pg_set_framecodes)", which);
        p.f.resize((size_t)(ns.n_codes + 1) * VW);
        for (int c = 0; c <= ns.n_codes; ++c)
            for (int o = 0; o < VW; ++o) {
                double s = 0.0;
                for (int k = 0; k < FC_CH; ++k) s += (double)t.view_w[(size_t)o * t.view_cols + W + CH_D + k] * (double)ns.codes_host[(size_t)c * FC_CH + k];
                p.f[(size_t)c * VW + o] = (float)s;
            }
        break;
    }
    case IMG_BIAS16: pgpack::pack_bias_s(t, p.f, src); break;
    case IMG_BIAS: pgpack::pack_bias(t, p.f); break;
    default: return pg_fail(h, PG_EINVAL, "no weight image %d", id);
    }
    return PG_OK;
}

// host memory -> a new device allocation; *d is set only once the copy has succeeded
int upload(pg_handle* h, const void* data, size_t bytes, void** d) {
    void* m = nullptr;
    PG_HIP(h, hipSetDevice(h->device));
    PG_HIP(h, hipMalloc(&m, bytes));
    const hipError_t e = hipMemcpy(m, data, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m);
        return pg_fail(h, PG_EHIP, "upload of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    *d = m;
    return PG_OK;
}

int refresh_host(pg_handle* h, int which);

// Image `id` of net `which` on the device, packed and uploaded by the first call that needs it.  A slot that exists is current:
// pg_load_weights releases them all, pg_load_weights_device all but those it re-forms (IMG_BIAS: see refresh_host)
int ensure_image(pg_handle* h, int which, int id) {
    NetState& ns = h->net[which];
    if (!ns.loaded) return pg_fail(h, PG_ESTATE, "weights of net %d not loaded", which);
    NetState::Slot& s = ns.img[id];
    if (s.d) return PG_OK;
    PG_TRY(refresh_host(h, which));     // (the last weights may have come from the device)
    Packed p;
    PG_TRY(pack_image(h, which, tensors_of(ns, h->cfg), id, p));     // (tensors_of folds feature_linear into the view layer: milliseconds of host work, once per load)
    PG_TRY(upload(h, p.data(), p.bytes(), reinterpret_cast<void**>(&s.d)));
    s.bytes = p.bytes();
    ++ns.builds;
    return PG_OK;
}

constexpr uint64_t image_bit(int id) { return 1ull << id; }
static_assert(IMG_COUNT <= 64, "release_images keeps by bit mask");

// Frees every image whose bit is not in `keep`; `sync`: one device synchronise in front when there is anything to free
// (without it hipFree itself waits for the device)
hipError_t release_images(NetState& ns, uint64_t keep, bool sync) {
    hipError_t first = hipSuccess;
    for (int id = 0; id < IMG_COUNT; ++id) {
        NetState::Slot& s = ns.img[id];
        if (!s.d || (keep & image_bit(id))) continue;
        if (sync) { first = hipDeviceSynchronize(); sync = false; }
        const hipError_t e = hipFree(s.d);
        if (first == hipSuccess) first = e;
        s = {};
    }
    return first;
}

// Everything a subject holds on the device (the caller has set the device); the subject is empty afterwards
void release_subject(Subject& sub) {
    for (NetState& ns : sub.net) {
        (void)release_images(ns, 0, false);
        if (ns.d_codes) (void)hipFree(ns.d_codes);
        if (ns.d_src) (void)hipFree(ns.d_src);
        for (int32_t* m : ns.d_map) if (m) (void)hipFree(m);
        if (ns.d_vwide) (void)hipFree(ns.d_vwide);
        ns = NetState();
    }
    if (sub.d_cut) (void)hipFree(sub.d_cut);
    sub.d_cut = nullptr;
}

// The host copies of a net's tensors are brought up to date if the last weights came from the device
// (pg_load_weights_device leaves them stale: only the images it re-forms itself are current) -- and with them the 32-row bias
// table, the one image that is kept over a device load without being re-formed there: the streams it goes with are all released
// by the load, so the first call that reads it comes through here first
int refresh_host(pg_handle* h, int which) {
    NetState& ns = h->net[which];
    if (!ns.host_stale) return PG_OK;
    pgpack::NetTensors lay;
    lay.layout(h->cfg.framecode_ch);
    PG_HIP(h, hipSetDevice(h->device));
    PG_HIP(h, hipDeviceSynchronize());
    for (int i = 0; i < 24; ++i)
        PG_HIP(h, hipMemcpy(ns.host[i].data(), ns.d_src + lay.off[i], ns.host[i].size() * sizeof(float), hipMemcpyDeviceToHost));
    ns.fold_w.clear(); ns.fold_b.clear();
    if (ns.d_codes && !ns.codes_host.empty())
        PG_HIP(h, hipMemcpy(ns.codes_host.data(), ns.d_codes, ns.codes_host.size() * sizeof(float), hipMemcpyDeviceToHost));
    ns.host_stale = false;
    PG_HIP(h, release_images(ns, ~image_bit(IMG_BIAS), false));
    return ensure_image(h, which, IMG_BIAS);
}

// the images form `f` reads at precision `prec`; the Yc table only `with_codes` (a launch with frame codes)
int ensure_form_images(pg_handle* h, int which, Form f, int prec, bool with_codes) {
    const FormInfo& fi = FORMS[f];
    for (const int image : {fi.stream, fi.wy, fi.bias}) {
        if (image == IMG_NONE || (image == IMG_YCODE && !with_codes)) continue;
        PG_TRY(ensure_image(h, which, image_of(image, prec)));
    }
    return PG_OK;
}

// the images a precision mode will use for net `which` in the usual call (usual_form), built ahead of the first render; the
// other forms of the mode (per-ray poses, short rays, explicit points) are packed by the first call that needs them
// (launch_eval_one), and so is the Yc table: the frame codes are set after the weights
int ensure_mode_streams(pg_handle* h, int which, int mode) {
    auto one = [&](int prec) { return ensure_form_images(h, which, usual_form(h, prec), prec, false); };
    if (mode != PG_PREC_FP16M) return one(mode);
    int rc = one(PG_PREC_FP16C);
    if (!rc && which == 0 && !h->cfg.single_net) rc = one(PG_PREC_FP16);      // (single_net: no guide pass)
    return rc;
}

// The images pg_load_weights_device re-forms on the device (pg_repack.hip), bitwise as pack_image would pack them: by a gather
// through a source map (built once, by pack_image in index mode) or, the Yc table, from the frame codes.  Every other image but
// IMG_BIAS is released by that load.
enum Gather { G_BF16, G_F16, G_F32, G_YCODE };
struct Reformed { int image, map, gather; const char* what; };
constexpr Reformed REFORMED[] = {
    {IMG_ONCHIP16 + PG_PREC_BF16, MAP_ONCHIP16, G_BF16, "the on-chip stream"},
    {IMG_ONCHIP16 + PG_PREC_FP16, MAP_ONCHIP16, G_F16, "the on-chip stream"},
    {IMG_C2, MAP_C2, G_F16, "the tile-split image"},
    {IMG_BIAS16, MAP_BIAS16, G_F32, "the 16-row bias table"},
    {IMG_YCODE, MAP_NONE, G_YCODE, "the frame-code table"},         // (behind pg_launch_codes: it reads the new codes)
};

int ensure_ws(pg_handle* h, size_t bytes) {
    if (bytes <= h->ws.bytes) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    return pg_grow(h, h->ws, bytes, "workspace allocation", bytes + bytes / 8);
}

int check_ready(pg_handle* h, bool need_fine) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    need_fine = need_fine && !h->cfg.single_net;        // single_net: network_fine is network (raycasters.py:99-104)
    if (!h->net[0].loaded) return pg_fail(h, PG_ESTATE, "coarse network weights not loaded (pg_load_weights)");
    if (need_fine && !h->net[1].loaded) return pg_fail(h, PG_ESTATE, "fine network weights not loaded (pg_load_weights)");
    if (!h->emb_set[0] || !h->emb_set[1]) return pg_fail(h, PG_ESTATE, "embedder state not set (pg_set_embedder)");
    return PG_OK;
}

// EvalArgs::skip_empty (pg_eval16r.hip): a wave whose points all have sigma <= 0 may leave the colour branch out only when
// nothing can tell -- `colour_free`: the caller composites the launch's raw without density noise and hands the raw itself
// to nobody (no raw output, no debug tap, not the training forward); the density is the ReLU one on a positive scale, so
// sigma <= 0 is alpha = 0 exactly (softplus is positive everywhere); and the switch is on (pg_set_empty_skip).
bool skip_empty_ok(const pg_handle* h, bool colour_free) {
    return colour_free && h->empty_skip && h->cfg.density_act == PG_ACT_RELU && h->cfg.density_scale > 0.0f;
}

// One launch of a net on n rays x S samples: what a caller of launch_eval fills in, by name (the arrays as pg_stage_eval takes them)
struct EvalCall {
    int which = 0;
    long long n = 0;
    int S = 0;
    const float *rays = nullptr, *z = nullptr, *skts = nullptr, *cams = nullptr;
    long long pose_stride = 0;
    float *raw = nullptr, *dbg = nullptr;
    int dbg_stage = 0;
    const float *points = nullptr, *pnoise = nullptr;       // [n S,3] explicit points instead of rays + z; [n,S,3] position noise
    bool guide_pass = false, colour_free = false;           // pass_precision; skip_empty_ok
    EvalCall slice(long long r0, long long m) const {       // rays [r0, r0 + m) of a call from rays (no points, no debug tap)
        EvalCall c = *this;
        c.n = m;
        c.rays += r0 * 11; c.z += r0 * S; c.skts += r0 * pose_stride; c.raw += r0 * S * 4;
        if (cams) c.cams += r0;
        if (pnoise) c.pnoise += r0 * S * 3;
        return c;
    }
};

// The launch of `what` between two events of the handle's pool while it profiles; the pair is filed into `list` (ev_used / ev_aux)
// unless the launch failed: a failed launch is not a sample.
template <typename F>
int timed_launch(pg_handle* h, void* stream, std::vector<std::pair<hipEvent_t, hipEvent_t>>& list, const char* what, F launch) {
    if (!h->profiling) { PG_TRY_LAUNCH(h, what, launch()); return PG_OK; }
    hipEvent_t ev[2];
    for (hipEvent_t& e : ev) {
        if (h->ev_free.empty()) PG_HIP(h, hipEventCreate(&e));
        else { e = h->ev_free.back(); h->ev_free.pop_back(); }
    }
    PG_HIP(h, hipEventRecord(ev[0], static_cast<hipStream_t>(stream)));
    const int err = launch();
    PG_HIP(h, hipEventRecord(ev[1], static_cast<hipStream_t>(stream)));
    if (err) { h->ev_free.push_back(ev[0]); h->ev_free.push_back(ev[1]); }
    else list.emplace_back(ev[0], ev[1]);
    PG_TRY_LAUNCH(h, what, err);
    return PG_OK;
}

int launch_eval_one(pg_handle* h, void* stream, EvalCall c) {
    const long long n = c.n;
    const int prec = pass_precision(h->cfg.precision, c.guide_pass);
    const bool fc = h->cfg.framecode_ch > 0;
    Form form = pick_form(CallFacts{prec, c.S, c.pose_stride, fc, c.points != nullptr, c.pnoise != nullptr, c.dbg != nullptr, c.dbg_stage, h->onchip_mode}, switches());
    // pg_debug_wave_counts: a launch of the on-chip form that the counting instantiation covers (one pose, no frame codes) adds
    // its counters to the caller's words -- what a render call's own launches did, not a stage call beside it
    if (!c.dbg && h->wave_counts && form == F_ONCHIP16 && c.pose_stride == 0 && !fc) { c.dbg = reinterpret_cast<float*>(h->wave_counts); c.dbg_stage = 97; }
    const FormInfo& fi = FORMS[form];
    const int y_bytes = fi.rec_y_bytes;
    PG_TRY(ensure_form_images(h, c.which, form, prec, fc));
    if (y_bytes) PG_TRY(ensure_rec(h, n, y_bytes));
    NetState& ns = h->net[c.which];
    if (fc && !ns.d_codes) return pg_fail(h, PG_ESTATE, "frame codes of net %d not set (pg_set_framecodes)", c.which);
    pgd::EvalArgs a{};
    a.rays = c.rays; a.z = c.z; a.pts = c.points; a.pnoise = c.pnoise; a.skts = c.skts; a.cams = c.cams;
    a.codes = fc ? ns.d_codes : nullptr;
    a.wstream = ns.img[image_of(fi.stream, prec)].d;
    a.wy = fi.wy == IMG_NONE || (fi.wy == IMG_YCODE && !fc) ? nullptr : ns.img[image_of(fi.wy, prec)].d;
    a.bias = reinterpret_cast<const float*>(ns.img[fi.bias].d);
    if (y_bytes) {
        a.rec_y = h->rec.p;
        a.rec_ab = reinterpret_cast<const float*>(h->rec.p + (size_t)(n + REC_PAD_RAYS) * y_bytes);
        // the padding rays behind the last record are fetched by the last passes (their values are multiplied by
        // zero weights at most): keep them finite whatever the buffer held before.  The record kernel writes rays
        // < n only, so the padding of an (n, record size) pair stays zero until another pair moves it.
        // (every writer of h->rec -- the record kernel -- stores rays < n only; anything else that is ever handed the
        // buffer must reset rec_pad_n to -1, as ensure_rec does)
        if (h->rec_pad_n != n || h->rec_pad_y != y_bytes || h->rec_pad_stream != stream) {
            PG_HIP(h, hipMemsetAsync(h->rec.p + (size_t)n * y_bytes, 0, (size_t)REC_PAD_RAYS * y_bytes, static_cast<hipStream_t>(stream)));
            PG_HIP(h, hipMemsetAsync(h->rec.p + (size_t)(n + REC_PAD_RAYS) * y_bytes + (size_t)n * REC_AB_BYTES, 0,
                                     (size_t)REC_PAD_RAYS * REC_AB_BYTES, static_cast<hipStream_t>(stream)));
            h->rec_pad_n = n; h->rec_pad_y = y_bytes; h->rec_pad_stream = stream;
        }
    }
    a.cutoff = h->d_cut;
    a.raw = c.raw; a.dbg = c.dbg;
    a.pose_stride = c.pose_stride;
    a.n_points = n * c.S;
    a.n_rays = (int)n;
    a.S = c.S;
    a.n_codes = ns.n_codes;
    a.tau_v = h->tau[0];
    a.tau_d = h->tau[1];
    a.dbg_stage = c.dbg_stage;
    a.far_skip = h->far_skip ? 1 : 0;
    a.skip_empty = skip_empty_ok(h, c.colour_free) ? 1 : 0;
    const int pts = fi.points_per_pass();
    if (!c.points && c.S < pts / (MAXR - 1))      // explicit points are one pseudo ray: a pass touches one slot
        return pg_fail(h, PG_EINVAL, "N_samples=%d too small: the fused kernel needs >= %d samples per ray", c.S, pts / (MAXR - 1));
    const long long iters = (a.n_points + pts - 1) / pts;
    a.n_iters = (int)iters;
    // POSEGEN_MAX_WG (measurement aid): fewer persistent workgroups than CUs, to see how much of a pass's time
    // is contention between CUs (the weight stream is pulled from L2 by every CU) rather than its own work
    static const long long wg_cap = [] { const char* e = std::getenv("POSEGEN_MAX_WG"); return e ? std::atoll(e) : 0ll; }();
    long long max_wg = (long long)h->n_cu * fi.wgs_per_cu();
    if (wg_cap > 0 && wg_cap < max_wg) max_wg = wg_cap;
    const int grid = (int)(iters < max_wg ? iters : max_wg);
    a.walk_rho = switches().pass_walk % grid;
    if (y_bytes) {          // what depends on the ray only, once per ray, in front of the fused kernel (pg_rayrec.hip)
        pgd::RecArgs ra{};
        ra.rays = c.rays; ra.skts = c.skts; ra.cams = c.cams; ra.codes = a.codes; ra.wy = a.wy;
        ra.rec_ab = const_cast<float*>(a.rec_ab); ra.rec_y = const_cast<uint8_t*>(a.rec_y);
        ra.pose_stride = c.pose_stride; ra.n_rays = (int)n; ra.n_codes = ns.n_codes;
        ra.z = c.z; ra.S = c.S;
        PG_TRY(timed_launch(h, stream, h->ev_aux, "ray record kernel", [&] {
            return pg_launch_ray_records(&ra, prec == PG_PREC_FP16, fc, h->n_cu, stream);
        }));
    }
    const int f16 = prec == PG_PREC_FP16;
    PG_TRY(timed_launch(h, stream, h->ev_used, "fused embed+MLP kernel", [&] {
        switch (form) {
        case F_DIRECT16:    return pg_launch_eval16(&a, f16, fc, grid, stream);
        case F_REC16:       return pg_launch_eval16r(&a, f16, fc, 0, grid, stream);
        case F_ONCHIP16:    return pg_launch_eval16r(&a, f16, fc, 1, grid, stream);
        case F_C2:          return pg_launch_evalc2(&a, fc, grid, stream);
        default:            return pg_launch_eval32(&a, prec, fc, grid, stream);
        }
    }));
    if (h->profiling) h->prof_points += a.n_points;
    return PG_OK;
}

// One net on n rays x S samples.  Calls with more than REC_BATCH_RAYS rays run as consecutive launches over ray
// ranges (rays are independent): the per-ray records (8.75 / 16.75 KiB per ray) then need 4.6 / 9 GB at most instead
// of growing with the call (a 2048 x 2048 frame would ask for 72 GB).  POSEGEN_REC_BATCH overrides the size (tests).
int launch_eval(pg_handle* h, void* stream, const EvalCall& c) {
    long long batch = 1ll << 19;
    if (const char* e = std::getenv("POSEGEN_REC_BATCH")) { const long long v = std::atoll(e); if (v >= 64) batch = v; }
    if (c.points || c.dbg || c.n <= batch) return launch_eval_one(h, stream, c);
    for (long long r0 = 0; r0 < c.n; r0 += batch) PG_TRY(launch_eval_one(h, stream, c.slice(r0, std::min(batch, c.n - r0))));
    return PG_OK;
}

// ---- argument rules that several entry points share ----
// the net a stage call names (`fn`: the entry point, for the message): ready, 0 or 1, and 0 on a single_net handle
int check_net(pg_handle* h, int which, const char* fn) {
    PG_TRY(check_ready(h, which == 1));
    if (which < 0 || which > 1) return pg_fail(h, PG_EINVAL, "%s: which_net must be 0 or 1", fn);
    if (which == 1 && h->cfg.single_net) return pg_fail(h, PG_EINVAL, "%s: a single_net handle has one net (which_net 0)", fn);
    return PG_OK;
}
// (`prefix`: "name: " or nothing, as the entry point has always worded it)
int check_samples(pg_handle* h, int S, int N, const char* prefix) {
    if (S < 2 || S > pg_composite_max_samples()) return pg_fail(h, PG_EINVAL, "%sN_samples %d outside [2,%d]", prefix, S, pg_composite_max_samples());
    if (N < 0 || N == 1 || N > pg_composite_max_importance())
        return pg_fail(h, PG_EINVAL, "%sN_importance %d outside {0, 2..%d}", prefix, N, pg_composite_max_importance());
    return PG_OK;
}

// the workspace of a call, carved by `carve` (pg_handle.h Carver): sized, grown if need be, then handed out
template <typename F> int carve_ws(pg_handle* h, F carve) {
    Carver sizes;
    carve(sizes);
    PG_TRY(ensure_ws(h, sizes.off));
    Carver c{h->ws.p};
    carve(c);
    return PG_OK;
}

}  // namespace

int pg_check_pose_stride(pg_handle* h, long long v, bool stage) {
    if (v == 0 || v == 384) return PG_OK;
    return pg_fail(h, PG_EINVAL, stage ? "pose_stride must be 0 or 384" : "pose_stride must be 0 (shared) or 384 (per ray)");
}
int pg_check_cyl_stride(pg_handle* h, long long v, bool stage) {
    if (v == 0 || v == 5) return PG_OK;
    return pg_fail(h, PG_EINVAL, stage ? "cyl_stride must be 0 or 5" : "cyl_stride must be 0 (shared) or 5 (per ray)");
}
int pg_check_joint_selection(pg_handle* h, const char* who, int J_in, const int32_t* joints, int* J, int root, bool once) {
    if (J_in < 1) return pg_fail(h, PG_EINVAL, "%s: J_in = %d", who, J_in);
    if (!joints) *J = J_in;
    if (*J < 1 || *J > PG_POSE_MAX_JOINTS) return pg_fail(h, PG_EINVAL, "%s: J = %d is outside [1, %d]", who, *J, PG_POSE_MAX_JOINTS);
    if (joints)
        for (int j = 0; j < *J; ++j) {
            if (joints[j] < 0 || joints[j] >= J_in) return pg_fail(h, PG_EINVAL, "%s: joints[%d] = %d is outside [0, %d)", who, j, joints[j], J_in);
            for (int k = 0; once && k < j; ++k)
                if (joints[k] == joints[j]) return pg_fail(h, PG_EINVAL, "%s: joints[%d] = joints[%d] = %d (a joint is selected once)", who, k, j, joints[j]);
        }
    if (root < -1 || root >= J_in) return pg_fail(h, PG_EINVAL, "%s: root = %d is outside [-1, %d)", who, root, J_in);
    return PG_OK;
}

int pg_sc_scratch(pg_handle* h, long long n, int chunk, double** out) {
    *out = nullptr;
    const long long need = pg_sample_coarse_scratch(n, chunk);
    if (need <= 0) return PG_OK;
    const size_t bytes = (size_t)need * sizeof(double);
    if (bytes > h->sc_part.bytes) {
        PG_HIP(h, hipSetDevice(h->device));
        PG_TRY(pg_grow(h, h->sc_part, bytes, "coarse sampler scratch", 2 * bytes));
    }
    *out = h->sc_part.as<double>();
    return PG_OK;
}

extern "C" {

int pg_abi_version(void) { return PG_ABI_VERSION; }

const char* pg_last_error(const pg_handle* h) { return h ? h->err : g_last_error; }

int pg_create(const pg_config* cfg, int n_devices, const int* device_ids, pg_handle** out) {
    if (!cfg || !out) return pg_fail(nullptr, PG_EINVAL, "pg_create: null argument");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return pg_fail(nullptr, PG_EINVAL, "pg_create: n_devices must be 1..64, got %d", n_devices);
    if (n_devices > 1 && !device_ids) return pg_fail(nullptr, PG_EINVAL, "pg_create: device_ids required for n_devices > 1");
    if (cfg->n_joints != J || cfg->multires != LV || (cfg->multires_views != LD && cfg->multires_views != 0) || cfg->multires_bones != 0 ||
        cfg->net_depth != DEPTH || cfg->net_width != W || cfg->skip_layer != SKIP || cfg->view_width != VW ||
        (cfg->framecode_ch != 0 && cfg->framecode_ch != FC_CH))
        return pg_fail(nullptr, PG_EINVAL,
                    "pg_create: unsupported architecture (kernels are built for 24 joints, multires 7/{4,0}/0, "
                    "8x256 trunk, skip 4, view width 128, frame code 0|16)");
    if (cfg->single_net != 0 && cfg->single_net != 1) return pg_fail(nullptr, PG_EINVAL, "pg_create: single_net must be 0 or 1, got %d", cfg->single_net);
    if (cfg->precision < 0 || cfg->precision >= PG_PREC_MODES) return pg_fail(nullptr, PG_EINVAL, "pg_create: bad precision %d", cfg->precision);
    if (is_x3(cfg->precision) && !x3_allowed())
        return pg_fail(nullptr, PG_EINVAL, "pg_create: split-operand precision %d is experimental (set POSEGEN_EXPERIMENTAL_X3=1)", cfg->precision);
    if (cfg->chunk <= 0) return pg_fail(nullptr, PG_EINVAL, "pg_create: chunk must be positive");
    if (!(cfg->density_scale > 0.f)) return pg_fail(nullptr, PG_EINVAL, "pg_create: density_scale must be positive");
    if (cfg->density_act != PG_ACT_RELU && cfg->density_act != PG_ACT_SOFTPLUS)
        return pg_fail(nullptr, PG_EINVAL, "pg_create: density_act must be PG_ACT_RELU or PG_ACT_SOFTPLUS, got %d", cfg->density_act);
    pg_handle* h = new (std::nothrow) pg_handle();
    if (h) { h->onchip_mode = switches().onchip; h->empty_skip = switches().empty_skip; }
    if (!h) return pg_fail(nullptr, PG_ENOMEM, "pg_create: out of host memory");
    h->cfg = *cfg;
    h->device = device_ids ? device_ids[0] : 0;
    for (int i = 0; i < 48; ++i) h->cut[i] = cfg->cutoff_dist;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { delete h; return pg_fail(nullptr, PG_EHIP, "pg_create: no HIP device available (%s)", hipGetErrorString(e)); }
    if (h->device < 0 || h->device >= ndev) { delete h; return pg_fail(nullptr, PG_EINVAL, "pg_create: device %d out of range (%d devices)", cfg ? device_ids ? device_ids[0] : 0 : 0, ndev); }
    hipDeviceProp_t prop;
    if (hipSetDevice(h->device) != hipSuccess || hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
        delete h;
        return pg_fail(nullptr, PG_EHIP, "pg_create: cannot query device");
    }
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->clock_khz = prop.clockRate;
    if (hipMalloc(reinterpret_cast<void**>(&h->d_cut), 48 * sizeof(float)) != hipSuccess) {
        delete h;
        return pg_fail(nullptr, PG_ENOMEM, "pg_create: device allocation failed");
    }
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        pg_destroy(h);
        return pg_fail(nullptr, PG_ENOMEM, "pg_create: stream creation failed");
    }
    // further devices: one sub-handle each (the same device may be listed twice: two workers on one GPU)
    for (int i = 1; i < n_devices; ++i) {
        pg_handle* sub = nullptr;
        const int rc = pg_create(cfg, 1, &device_ids[i], &sub);
        if (rc) { pg_destroy(h); return rc; }
        h->peers.push_back(sub);
    }
    // The gather of a cut frame (pg_render_frames phase B) is a device-to-device copy: it goes over xGMI only
    // with peer access enabled in both directions, otherwise the runtime stages it through the host -- refused
    // here rather than done silently (POSEGEN_ALLOW_STAGED_PEER=1 accepts the staged copies).
    if (n_devices > 1) {
        const char* ev = std::getenv("POSEGEN_ALLOW_STAGED_PEER");
        const bool allow_staged = ev && ev[0] == '1';
        for (int i = 0; i < n_devices; ++i)
            for (int j = 0; j < n_devices; ++j) {
                const int di = device_ids[i], dj = device_ids[j];
                if (di == dj) continue;
                int can = 0;
                hipError_t pe = hipDeviceCanAccessPeer(&can, di, dj);
                if (pe == hipSuccess && can) {
                    pe = hipSetDevice(di);
                    if (pe == hipSuccess) pe = hipDeviceEnablePeerAccess(dj, 0);
                    if (pe == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); pe = hipSuccess; }
                }
                if ((pe != hipSuccess || !can) && !allow_staged) {
                    const int rc = pg_fail(nullptr, PG_EHIP, "pg_create: device %d cannot access device %d directly (%s); frame gathers would be "
                                        "staged through the host (set POSEGEN_ALLOW_STAGED_PEER=1 to accept that)", di, dj,
                                        pe != hipSuccess ? hipGetErrorString(pe) : "hipDeviceCanAccessPeer = 0");
                    pg_destroy(h);
                    return rc;
                }
            }
        (void)hipSetDevice(h->device);
    }
    *out = h;
    return PG_OK;
}

void pg_destroy(pg_handle* h) {
    if (!h) return;
    for (pg_handle* sub : h->peers) pg_destroy(sub);
    h->peers.clear();
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    for (DevBuf* b : {&h->fws, &h->rec, &h->sc_part}) pg_release(*b);
    // the modules' states, in slot order; their destructors free device memory, streams and events of h->device, which is current
    // here (no module sets the device again)
    h->mods.clear();
    for (auto& pr : h->ev_aux) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    release_subject(*h);
    for (Subject& sub : h->bank.parked) release_subject(sub);
    for (auto& pr : h->ev_used) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& ev : h->ev_free) (void)hipEventDestroy(ev);
    pg_release(h->ws);
    delete h;
}

int pg_load_weights(pg_handle* h, int which, const float* const* tensors, const int64_t* shapes, int n_tensors) {
    if (!h || !tensors || !shapes) return pg_fail(h, PG_EINVAL, "pg_load_weights: null argument");
    if (which < 0 || which > 1) return pg_fail(h, PG_EINVAL, "pg_load_weights: which_net must be 0 or 1");
    if (n_tensors != 24) return pg_fail(h, PG_EINVAL, "pg_load_weights: expected 24 tensors, got %d", n_tensors);
    if (which == 1 && h->cfg.single_net) return pg_fail(h, PG_EINVAL, "pg_load_weights: a single_net handle has one net (which_net 0)");
    const bool views0 = h->cfg.multires_views == 0;
    const int vcols = W + (views0 ? CH_D0 : CH_D) + h->cfg.framecode_ch;
    int64_t want[24][2];
    for (int l = 0; l < DEPTH; ++l) {
        want[2 * l][0] = W; want[2 * l][1] = l == 0 ? CH_X : (l == SKIP + 1 ? CH_X + W : W);
        want[2 * l + 1][0] = W; want[2 * l + 1][1] = 1;
    }
    want[16][0] = 1; want[16][1] = W;       want[17][0] = 1; want[17][1] = 1;
    want[18][0] = W; want[18][1] = W;       want[19][0] = W; want[19][1] = 1;
    want[20][0] = VW; want[20][1] = vcols;  want[21][0] = VW; want[21][1] = 1;
    want[22][0] = 3; want[22][1] = VW;      want[23][0] = 3; want[23][1] = 1;
    for (int i = 0; i < 24; ++i) {
        if (!tensors[i]) return pg_fail(h, PG_EINVAL, "pg_load_weights: tensor %d is null", i);
        if (shapes[2 * i] != want[i][0] || shapes[2 * i + 1] != want[i][1])
            return pg_fail(h, PG_EINVAL, "pg_load_weights: tensor %d has shape [%lld,%lld], expected [%lld,%lld]", i,
                        (long long)shapes[2 * i], (long long)shapes[2 * i + 1], (long long)want[i][0], (long long)want[i][1]);
    }
    NetState& ns = h->net[which];
    static const bool time_load = std::getenv("POSEGEN_TIME_LOAD") != nullptr;
    const auto tl0 = std::chrono::steady_clock::now();
    ns.host.assign(24, {});
    ns.fold_w.clear(); ns.fold_b.clear();
    for (int i = 0; i < 24; ++i) ns.host[i].assign(tensors[i], tensors[i] + want[i][0] * want[i][1]);
    if (views0) {       // every image, fold and record below sees the 4-band matrix
        ns.host[20].assign((size_t)VW * (W + CH_D + h->cfg.framecode_ch), 0.0f);
        widen_view_w(tensors[20], h->cfg.framecode_ch, ns.host[20].data());
    }
    ns.loaded = true;
    ns.host_stale = false;
    PG_HIP(h, hipSetDevice(h->device));
    PG_HIP(h, release_images(ns, 0, true));
    if (const int rc = ensure_image(h, which, IMG_BIAS)) return rc;
    const auto tl1 = std::chrono::steady_clock::now();
    const int rc0 = ensure_mode_streams(h, which, h->cfg.precision);
    if (rc0) return rc0;
    if (time_load) {
        const auto tl2 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "pg_load_weights net %d: copy + free + fold + bias %.2f ms, stream of the mode %.2f ms\n", which,
                     std::chrono::duration<double, std::milli>(tl1 - tl0).count(), std::chrono::duration<double, std::milli>(tl2 - tl1).count());
    }
    PG_FORWARD(h, pg_load_weights(hh, which, tensors, shapes, n_tensors));
    return PG_OK;
}

// New values for a loaded net's tensors (and frame codes) from DEVICE memory -- what sits between optimiser steps and a
// validation render (TrainableRayCaster.sync_inference_weights; the reference renders with the module it trains,
// core/trainer.py:463).  The images of the fast paths -- the on-chip stream of the 16x16x32 kernel (bf16 / fp16), pg_evalc2.hip's
// weight image, their bias table, the frame-code tables: REFORMED -- are re-formed on the device, bitwise as pg_load_weights would pack
// them (pg_repack.hip); every other image is dropped and re-packed from the host copies, which are refreshed from the device,
// by the first call that needs it.  Enqueued on `stream`; the tensors may be reused as soon as the call returns in stream order.
int pg_load_weights_device(pg_handle* h, void* stream, int which, const float* const* d_tensors, int n_tensors, const float* d_codes, int n_codes) {
    if (!h || !d_tensors) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: null argument");
    if (which < 0 || which > 1) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: which_net must be 0 or 1");
    if (which == 1 && h->cfg.single_net) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: a single_net handle has one net (which_net 0)");
    if (n_tensors != 24) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: expected 24 tensors, got %d", n_tensors);
    if (!h->peers.empty()) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: a multi-device handle takes its weights from the host (pg_load_weights)");
    NetState& ns = h->net[which];
    if (!ns.loaded) return pg_fail(h, PG_ESTATE, "pg_load_weights_device: net %d has no weights yet (the first load is pg_load_weights: it fixes the shapes)", which);
    const bool fc = h->cfg.framecode_ch > 0;
    if (fc && (!d_codes || n_codes != ns.n_codes || !ns.d_codes))
        return pg_fail(h, PG_EINVAL, "pg_load_weights_device: frame codes [%d,16] expected (set once by pg_set_framecodes)", ns.n_codes);
    for (int i = 0; i < 24; ++i)
        if (!d_tensors[i]) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: tensor %d is null", i);
    PG_HIP(h, hipSetDevice(h->device));
    pgpack::NetTensors lay;                                 // (offsets only; a source map is built from the shapes, see map_tensors)
    lay.layout(h->cfg.framecode_ch);
    auto map_tensors = [&]() {      // the packers in index mode: pointers and shapes as usual, the (possibly stale) values are not what is recorded
        pgpack::NetTensors t = tensors_of(ns, h->cfg);
        t.layout(h->cfg.framecode_ch);
        return t;
    };
    if (!ns.d_src) PG_HIP(h, hipMalloc(reinterpret_cast<void**>(&ns.d_src), (size_t)lay.off[pgpack::NetTensors::N_SRC] * sizeof(float)));
    const int vcols = W + CH_D + h->cfg.framecode_ch;
    const float* tens[24];
    for (int i = 0; i < 24; ++i) tens[i] = d_tensors[i];
    if (h->cfg.multires_views == 0) {       // the caller's [128, 256+72(+fc)] view weight, widened as pg_load_weights does
        if (!ns.d_vwide) PG_HIP(h, hipMalloc(reinterpret_cast<void**>(&ns.d_vwide), (size_t)VW * vcols * sizeof(float)));
        pg_launch_widen_views(d_tensors[20], h->cfg.framecode_ch, ns.d_vwide, stream);
        tens[20] = ns.d_vwide;
    }
    pg_launch_collect(tens, lay.off, ns.d_src, stream);        // (off[24] = the end of tensor 23: the folded view layer follows)
    pg_launch_fold(ns.d_src, lay.off[20], vcols, lay.off[21], lay.off[18], lay.off[19], lay.off[pgpack::NetTensors::SRC_VIEWF_W],
                   lay.off[pgpack::NetTensors::SRC_VIEWF_B], stream);
    // images re-formed here (those that exist: the others are built by the first call that needs them)
    if (fc) pg_launch_codes(d_codes, ns.n_codes, ns.d_codes, stream);
    uint64_t keep = image_bit(IMG_BIAS);                // (stale until refresh_host re-forms it)
    for (const Reformed& r : REFORMED) {
        const NetState::Slot& im = ns.img[r.image];
        keep |= image_bit(r.image);
        if (!im.d) continue;
        if (r.map != MAP_NONE && !ns.d_map[r.map]) {
            Packed p; std::vector<int32_t> m;
            if (pack_image(h, which, map_tensors(), r.image, p, &m)) return pg_fail(h, PG_EINVAL, "pg_load_weights_device: source map of %s", r.what);
            if (const int rc = upload(h, m.data(), m.size() * sizeof(int32_t), reinterpret_cast<void**>(&ns.d_map[r.map]))) return rc;
        }
        switch (r.gather) {
        case G_BF16: case G_F16:
            pg_launch_gather16(ns.d_map[r.map], ns.d_src, reinterpret_cast<uint16_t*>(im.d), (long long)(im.bytes / 2), r.gather == G_BF16, stream);
            break;
        case G_F32: pg_launch_gather32(ns.d_map[r.map], ns.d_src, reinterpret_cast<float*>(im.d), (long long)(im.bytes / 4), stream); break;
        case G_YCODE: pg_launch_ycode(ns.d_src + lay.off[20], vcols, ns.d_codes, ns.n_codes, reinterpret_cast<float*>(im.d), stream); break;
        }
        ++ns.builds;
    }
    PG_HIP(h, hipGetLastError());
    // everything else: dropped (hipFree waits for the device: only forms the run has used beside the fast paths pay it)
    (void)release_images(ns, keep, false);
    ns.fold_w.clear(); ns.fold_b.clear();
    ns.host_stale = true;               // (refresh_host also re-forms IMG_BIAS, the bias table of the other kernels)
    return ensure_mode_streams(h, which, h->cfg.precision);
}

int pg_set_embedder(pg_handle* h, int which, const float* cutoff_dist, float tau) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_embedder: null handle");
    if (which < 0 || which > 1) return pg_fail(h, PG_EINVAL, "pg_set_embedder: which must be 0 (embed_fn) or 1 (embeddirs_fn)");
    if (cutoff_dist) std::memcpy(h->cut + 24 * which, cutoff_dist, 24 * sizeof(float));
    h->tau[which] = tau;
    h->emb_set[which] = true;
    PG_HIP(h, hipSetDevice(h->device));
    PG_HIP(h, hipMemcpy(h->d_cut, h->cut, sizeof h->cut, hipMemcpyHostToDevice));
    PG_FORWARD(h, pg_set_embedder(hh, which, cutoff_dist, tau));
    return PG_OK;
}

int pg_set_framecodes(pg_handle* h, int which, const float* codes, int n_codes) {
    if (!h || !codes) return pg_fail(h, PG_EINVAL, "pg_set_framecodes: null argument");
    if (which < 0 || which > 1) return pg_fail(h, PG_EINVAL, "pg_set_framecodes: which_net must be 0 or 1");
    if (h->cfg.framecode_ch != FC_CH) return pg_fail(h, PG_EINVAL, "pg_set_framecodes: handle was created without frame codes");
    if (n_codes <= 0) return pg_fail(h, PG_EINVAL, "pg_set_framecodes: n_codes must be positive");
    NetState& ns = h->net[which];
    ns.codes_host.assign(codes, codes + (size_t)n_codes * FC_CH);
    ns.codes_host.resize((size_t)(n_codes + 1) * FC_CH, 0.f);
    for (int c = 0; c < FC_CH; ++c) {       // mean row (embedding.py:25-26), summed in row order
        float s = 0.f;
        for (int i = 0; i < n_codes; ++i) s += codes[(size_t)i * FC_CH + c];
        ns.codes_host[(size_t)n_codes * FC_CH + c] = s / (float)n_codes;
    }
    ns.n_codes = n_codes;
    PG_HIP(h, hipSetDevice(h->device));
    if (ns.d_codes) { PG_HIP(h, hipDeviceSynchronize()); PG_HIP(h, hipFree(ns.d_codes)); ns.d_codes = nullptr; }
    PG_HIP(h, release_images(ns, ~image_bit(IMG_YCODE), false));
    PG_HIP(h, hipMalloc(reinterpret_cast<void**>(&ns.d_codes), ns.codes_host.size() * sizeof(float)));
    PG_HIP(h, hipMemcpy(ns.d_codes, ns.codes_host.data(), ns.codes_host.size() * sizeof(float), hipMemcpyHostToDevice));
    PG_FORWARD(h, pg_set_framecodes(hh, which, codes, n_codes));
    return PG_OK;
}

// ---- the subject bank (pg_bank.h) ---------------------------------------------------------------------------------
int pg_subject_count(const pg_handle* h) { return h ? bank_count(h->bank) : 0; }

int pg_set_subject_count(pg_handle* h, int n) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_subject_count: null handle");
    if (n < 1 || n > PG_MAX_SUBJECTS) return pg_fail(h, PG_EINVAL, "pg_set_subject_count: 1..%d subjects, got %d", PG_MAX_SUBJECTS, n);
    if (h->tape_out) return pg_fail(h, PG_EINVAL, "pg_set_subject_count: a training tape is outstanding (run its backward first)");
    if (n <= h->bank.active)
        return pg_fail(h, PG_EINVAL, "pg_set_subject_count: subject %d is selected and would be dropped (select one below %d first)", h->bank.active, n);
    const int have = bank_count(h->bank);
    if (n != have) {
        PG_HIP(h, hipSetDevice(h->device));
        if (n < have) PG_HIP(h, hipDeviceSynchronize());       // (launches in flight may still read the dropped subjects' images)
        auto make = [&](Subject& sub) -> int {
            for (float& c : sub.cut) c = h->cfg.cutoff_dist;
            return hipMalloc(reinterpret_cast<void**>(&sub.d_cut), sizeof sub.cut) == hipSuccess ? PG_OK : PG_ENOMEM;
        };
        if (const int rc = bank_resize(*h, h->bank, n, make, release_subject)) return pg_fail(h, rc, "pg_set_subject_count: device allocation failed");
    }
    PG_FORWARD(h, pg_set_subject_count(hh, n));
    return PG_OK;
}

int pg_select_subject(pg_handle* h, int s) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_select_subject: null handle");
    if (s < 0 || s >= bank_count(h->bank)) return pg_fail(h, PG_EINVAL, "pg_select_subject: subject %d of %d", s, bank_count(h->bank));
    if (h->tape_out) return pg_fail(h, PG_EINVAL, "pg_select_subject: a training tape is outstanding (run its backward first; training a bank is not built)");
    bank_select(*h, h->bank, s);
    PG_FORWARD(h, pg_select_subject(hh, s));
    return PG_OK;
}

int pg_subject_info(pg_handle* h, int s, int32_t* loaded_nets, int64_t* image_bytes, int64_t* image_builds) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_subject_info: null handle");
    if (s < 0 || s >= bank_count(h->bank)) return pg_fail(h, PG_EINVAL, "pg_subject_info: subject %d of %d", s, bank_count(h->bank));
    const Subject& sub = s == h->bank.active ? static_cast<const Subject&>(*h) : h->bank.parked[s];
    int32_t loaded = 0;
    int64_t bytes = 0, builds = 0;
    for (int w = 0; w < 2; ++w) {
        const NetState& ns = sub.net[w];
        if (ns.loaded) loaded |= 1 << w;
        for (const NetState::Slot& im : ns.img) if (im.d) bytes += (int64_t)im.bytes;
        builds += ns.builds;
    }
    if (loaded_nets) *loaded_nets = loaded;
    if (image_bytes) *image_bytes = bytes;
    if (image_builds) *image_builds = builds;
    return PG_OK;
}

int pg_set_precision(pg_handle* h, int precision) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_precision: null handle");
    if (precision < 0 || precision >= PG_PREC_MODES) return pg_fail(h, PG_EINVAL, "pg_set_precision: bad precision %d", precision);
    if (is_x3(precision) && !x3_allowed())
        return pg_fail(h, PG_EINVAL, "pg_set_precision: split-operand precision %d is experimental (set POSEGEN_EXPERIMENTAL_X3=1)", precision);
    h->cfg.precision = precision;
    for (int w = 0; w < 2; ++w)
        if (h->net[w].loaded) { int rc = ensure_mode_streams(h, w, precision); if (rc) return rc; }
    PG_FORWARD(h, pg_set_precision(hh, precision));
    return PG_OK;
}

int pg_set_chunk(pg_handle* h, int chunk) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_chunk: null handle");
    if (chunk <= 0) return pg_fail(h, PG_EINVAL, "pg_set_chunk: chunk must be positive, got %d", chunk);
    h->cfg.chunk = chunk;
    PG_FORWARD(h, pg_set_chunk(hh, chunk));
    return PG_OK;
}

int pg_set_far_skip(pg_handle* h, int on) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_far_skip: null handle");
    h->far_skip = on != 0;
    PG_FORWARD(h, pg_set_far_skip(hh, on));
    return PG_OK;
}

int pg_set_empty_skip(pg_handle* h, int on) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_empty_skip: null handle");
    h->empty_skip = on != 0;
    PG_FORWARD(h, pg_set_empty_skip(hh, on));
    return PG_OK;
}

int pg_debug_wave_counts(pg_handle* h, uint32_t* counts) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_debug_wave_counts: null handle");
    h->wave_counts = counts;        // (this handle's device only: the peers of pg_render_frames do not count)
    return PG_OK;
}

int pg_set_onchip(pg_handle* h, int mode) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_set_onchip: null handle");
    if (mode < PG_ONCHIP_RECORDS || mode > PG_ONCHIP_ALWAYS) return pg_fail(h, PG_EINVAL, "pg_set_onchip: mode must be 0 (records), 1 (by sample count) or 2 (on chip), got %d", mode);
    h->onchip_mode = mode;
    PG_FORWARD(h, pg_set_onchip(hh, mode));
    return PG_OK;
}

int pg_set_train_precision(pg_handle* h, int precision) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (precision != PG_PREC_FP32 && precision != PG_PREC_BF16)
        return pg_fail(h, PG_EINVAL, "pg_set_train_precision: the training step computes in fp32 (PG_PREC_FP32) or on a bf16 tape (PG_PREC_BF16), not %d", precision);
    h->train_precision = precision;
    for (pg_handle* p : h->peers) p->train_precision = precision;
    return PG_OK;
}

int pg_profile_enable(pg_handle* h, int on) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_profile_enable: null handle");
    h->profiling = on != 0;
    return PG_OK;
}

// the record-kernel events recorded so far -> the handle's running totals; the events go back to the pool (called by
// both reads, so that a caller that only ever reads the fused kernel's numbers does not pile events up)
static int fold_aux(pg_handle* h) {
    for (auto& pr : h->ev_aux) {
        PG_HIP(h, hipEventSynchronize(pr.second));
        float t = 0.f;
        PG_HIP(h, hipEventElapsedTime(&t, pr.first, pr.second));
        h->aux_ms += t;
        h->aux_n += 1;
        h->ev_free.push_back(pr.first);
        h->ev_free.push_back(pr.second);
    }
    h->ev_aux.clear();
    return PG_OK;
}

int pg_profile_read_aux(pg_handle* h, int64_t* n_launches, double* total_ms) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_profile_read_aux: null handle");
    PG_HIP(h, hipSetDevice(h->device));
    if (const int rc = fold_aux(h)) return rc;
    if (n_launches) *n_launches = h->aux_n;
    if (total_ms) *total_ms = h->aux_ms;
    h->aux_n = 0;
    h->aux_ms = 0.0;
    return PG_OK;
}

int pg_profile_read(pg_handle* h, int64_t* n_launches, double* total_ms, int64_t* n_points) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_profile_read: null handle");
    PG_HIP(h, hipSetDevice(h->device));
    double ms = 0.0;
    for (auto& pr : h->ev_used) {
        PG_HIP(h, hipEventSynchronize(pr.second));
        float t = 0.f;
        PG_HIP(h, hipEventElapsedTime(&t, pr.first, pr.second));
        ms += t;
        h->ev_free.push_back(pr.first);
        h->ev_free.push_back(pr.second);
    }
    if (n_launches) *n_launches = (int64_t)h->ev_used.size();
    if (total_ms) *total_ms = ms;
    if (n_points) *n_points = h->prof_points;
    h->ev_used.clear();
    h->prof_points = 0;
    return fold_aux(h);             // (kept for the next pg_profile_read_aux)
}

int pg_debug_pack(const float* const* tensors, const int64_t* shapes, int n_tensors, int framecode_ch,
                  int precision, int view_fact, uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes, float* bias_out,
                  int32_t* chunk_bytes) {
    if (!tensors || !shapes || n_tensors != 24) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack: need 24 tensors");
    if (precision < 0 || precision >= PG_PREC_COUNT) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack: bad precision");
    NetState ns;
    host_copy(ns, tensors, shapes, framecode_ch);
    pg_config cfg{};
    cfg.framecode_ch = framecode_ch;
    std::vector<uint8_t> packed;
    const bool rprog = view_fact != 0 && is_shape_a(precision);       // the 16x16x32 program of pg_eval16r.hip
    const bool c2 = view_fact == 4 && precision == PG_PREC_FP16C;       // the weight image of pg_evalc2.hip (pg_program.h T)
    if (view_fact != 0 && !rprog && !c2)
        return pg_fail(nullptr, PG_EINVAL, precision == PG_PREC_FP16C ? "pg_debug_pack: PG_PREC_FP16C packs view_fact 0 (the k-major stream of pg_eval32.hip) or 4 (the image of pg_evalc2.hip), not %d"
                                                                      : "pg_debug_pack: this precision packs view_fact 0 (its k-major stream) only, not %d", view_fact);
    const int rc = c2 ? pgpack::pack_c2(tensors_of(ns, cfg), framecode_ch > 0, packed)
                 : rprog ? pgpack::pack_stream_r(tensors_of(ns, cfg), precision, packed, view_fact == 3)
                         : pgpack::pack_stream(tensors_of(ns, cfg), precision, framecode_ch > 0, packed);
    if (rc != 0) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack: packing failed (%d)", rc);
    if (stream_bytes) *stream_bytes = (int64_t)packed.size();
    if (chunk_bytes) *chunk_bytes = CHUNK_BYTES;
    if (stream_out) {
        if ((int64_t)packed.size() > stream_cap) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack: buffer too small");
        std::memcpy(stream_out, packed.data(), packed.size());
    }
    if (bias_out) {
        std::vector<float> bias;
        if (rprog || c2) pgpack::pack_bias_s(tensors_of(ns, cfg), bias);
        else pgpack::pack_bias(tensors_of(ns, cfg), bias);
        std::memcpy(bias_out, bias.data(), bias.size() * sizeof(float));
    }
    return PG_OK;
}

// Host-only: the source map of a packed image (pg_load_weights_device re-forms the image from it by a gather) and the flat
// source vector it indexes.  form 0: on-chip stream of the 16x16x32 kernel, 1: pg_evalc2.hip's image, 2: the 16-row bias table.
int pg_debug_pack_map(const float* const* tensors, const int64_t* shapes, int n_tensors, int framecode_ch, int form,
                      int32_t* map_out, int64_t map_cap, int64_t* map_n, float* src_out, int64_t src_cap, int64_t* src_n) {
    if (!tensors || !shapes || n_tensors != 24) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_map: need 24 tensors");
    NetState ns;
    host_copy(ns, tensors, shapes, framecode_ch);
    pg_config cfg{};
    cfg.framecode_ch = framecode_ch;
    pgpack::NetTensors t = tensors_of(ns, cfg);
    t.layout(framecode_ch);
    std::vector<int32_t> m;
    std::vector<uint8_t> img;
    std::vector<float> b;
    int rc = 0;
    if (form == 0) rc = pgpack::pack_stream_r(t, PG_PREC_BF16, img, true, &m);
    else if (form == 1) rc = pgpack::pack_c2(t, framecode_ch > 0, img, &m);
    else if (form == 2) pgpack::pack_bias_s(t, b, &m);
    else return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_map: form 0, 1 or 2");
    if (rc != 0) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_map: packing failed (%d)", rc);
    const int64_t ns_ = t.off[pgpack::NetTensors::N_SRC];
    if (map_n) *map_n = (int64_t)m.size();
    if (src_n) *src_n = ns_;
    if (map_out) {
        if ((int64_t)m.size() > map_cap) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_map: map buffer too small");
        std::memcpy(map_out, m.data(), m.size() * sizeof(int32_t));
    }
    if (src_out) {
        if (ns_ > src_cap) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_map: source buffer too small");
        for (int i = 0; i < 24; ++i) std::memcpy(src_out + t.off[i], ns.host[i].data(), ns.host[i].size() * sizeof(float));
        std::memcpy(src_out + t.off[pgpack::NetTensors::SRC_VIEWF_W], t.viewf_w.data(), t.viewf_w.size() * sizeof(float));
        std::memcpy(src_out + t.off[pgpack::NetTensors::SRC_VIEWF_B], t.viewf_b.data(), t.viewf_b.size() * sizeof(float));
    }
    return PG_OK;
}

int pg_debug_widen_views(const float* view_w, int64_t rows, int64_t cols, int framecode_ch, float* out, int64_t cap,
                         int64_t* out_n) {
    if (!view_w) return pg_fail(nullptr, PG_EINVAL, "pg_debug_widen_views: null argument");
    if (framecode_ch != 0 && framecode_ch != FC_CH) return pg_fail(nullptr, PG_EINVAL, "pg_debug_widen_views: frame code 0 or 16");
    if (rows != VW || cols != W + CH_D0 + framecode_ch)
        return pg_fail(nullptr, PG_EINVAL, "pg_debug_widen_views: view weight [%lld,%lld], expected [%d,%d]", (long long)rows,
                       (long long)cols, VW, W + CH_D0 + framecode_ch);
    const int64_t need = (int64_t)VW * (W + CH_D + framecode_ch);
    if (out_n) *out_n = need;
    if (out) {
        if (cap < need) return pg_fail(nullptr, PG_EINVAL, "pg_debug_widen_views: buffer too small");
        widen_view_w(view_w, framecode_ch, out);
    }
    return PG_OK;
}

// Test aid (not in the header): every workgroup of a grid of G walks its passes of an (n_rays, S) call through pgd::PassWalk on the
// host.  Returns the number of passes whose (first point, ray, sample) differ from the integer division plus the number of passes not
// taken exactly once; -1: bad arguments.
extern "C" long long pg_debug_pass_walk(long long n_rays, int S, int pts, int G, int rho) {
    if (n_rays <= 0 || S <= 0 || pts <= 0 || G <= 0 || rho < 0 || rho >= G) return -1;
    const long long n_iters = (n_rays * S + pts - 1) / pts;
    std::vector<uint8_t> taken((size_t)n_iters, 0);
    long long bad = 0;
    for (int b = 0; b < G; ++b) {
        int prev = -1;
        for (pgd::PassWalk w(S, pts, b, G, rho); w.it < n_iters; w.advance(), w.peek()) {
            const long long p0 = (long long)w.it * pts;
            if (w.p0 != p0 || w.r0 != p0 / S || w.off0 != p0 % S || w.it <= prev || w.it / G != w.itn / G - 1 || taken[(size_t)w.it]) ++bad;
            taken[(size_t)w.it] = 1;
            prev = w.it;
        }
    }
    for (long long i = 0; i < n_iters; ++i) bad += !taken[(size_t)i];
    return bad;
}

int pg_debug_pack_vy(const float* const* tensors, const int64_t* shapes, int n_tensors, int framecode_ch,
                     int precision, uint8_t* out, int64_t cap, int64_t* out_bytes) {
    if (!tensors || !shapes || n_tensors != 24) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_vy: need 24 tensors");
    NetState ns;
    host_copy(ns, tensors, shapes, framecode_ch);
    pg_config cfg{};
    cfg.framecode_ch = framecode_ch;
    std::vector<uint8_t> vy;
    if (pgpack::pack_vy(tensors_of(ns, cfg), precision, framecode_ch > 0, vy) != 0)
        return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_vy: 16-bit precisions only");
    if (out_bytes) *out_bytes = (int64_t)vy.size();
    if (out) {
        if ((int64_t)vy.size() > cap) return pg_fail(nullptr, PG_EINVAL, "pg_debug_pack_vy: buffer too small");
        std::memcpy(out, vy.data(), vy.size());
    }
    return PG_OK;
}

int pg_device_info(const pg_handle* h, int32_t* n_cu, int32_t* clock_khz) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_device_info: null handle");
    if (n_cu) *n_cu = h->n_cu;
    if (clock_khz) *clock_khz = h->clock_khz;
    return PG_OK;
}

int pg_calibrate_mfma(pg_handle* h, int f16, int lds_fed, double min_ms, double* tflops, double* ms_out) {
    if (!h || !tflops) return pg_fail(h, PG_EINVAL, "pg_calibrate_mfma: null argument");
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(ensure_ws(h, 256));
    hipEvent_t e0, e1;
    PG_HIP(h, hipEventCreate(&e0));
    PG_HIP(h, hipEventCreate(&e1));
    hipStream_t s = h->own_stream ? h->own_stream : nullptr;
    PG_HIP(h, hipDeviceSynchronize());                  // own_stream is not ordered behind the caller's stream, and ws is shared
    int blocks = h->n_cu;                               // POSEGEN_MAX_WG: fewer CUs (how the clock answers to the load)
    if (const char* e = std::getenv("POSEGEN_MAX_WG")) { const int c = std::atoi(e); if (c > 0 && c < blocks) blocks = c; }
    int iters = 2000;                                   // ~1 ms per 1000 iterations of 32 MFMAs at 2 waves/SIMD
    int timed_iters = 0;                                // iterations of the launch `ms` belongs to
    float ms = 0.0f;
    int err = 0;
    hipError_t herr = hipSuccess;
    for (int round = 0; round < 6; ++round) {           // grow until one launch lasts min_ms: the clock settles in ms
        (void)hipEventRecord(e0, s);
        err = pg_launch_mfma_rate(f16, lds_fed, blocks, iters, h->ws.as<float>(), s);
        (void)hipEventRecord(e1, s);
        if (err) break;
        herr = hipEventSynchronize(e1);
        if (herr == hipSuccess) herr = hipEventElapsedTime(&ms, e0, e1);
        if (herr != hipSuccess) break;
        timed_iters = iters;
        if (ms >= min_ms && round > 0) break;
        if (ms < min_ms) iters = (int)(iters * (ms > 0.05 ? 1.25 * min_ms / ms : 8.0)) + 1;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err) return pg_fail(h, PG_EHIP, "calibration launch failed: %s", hipGetErrorString((hipError_t)err));
    if (herr != hipSuccess) return pg_fail(h, PG_EHIP, "calibration kernel failed: %s", hipGetErrorString(herr));
    if (!(ms > 0.0f) || timed_iters <= 0) return pg_fail(h, PG_EHIP, "calibration measured no time (%.3f ms over %d iterations)", ms, timed_iters);
    const double flop = (double)blocks * 8.0 * (double)timed_iters * 32.0 * 32768.0;
    *tflops = flop / (ms * 1e-3) / 1e12;
    if (ms_out) *ms_out = ms;
    return PG_OK;
}

int pg_query(const pg_handle* h, int precision, int64_t* stream_bytes, int64_t* mfma_per_group) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "pg_query: null handle");
    if (precision < 0 || precision >= PG_PREC_MODES) return PG_EINVAL;
    if (precision == PG_PREC_FP16M) precision = PG_PREC_FP16C;      // the pass that produces the returned maps
    const FormInfo& fi = FORMS[usual_form(h, precision)];
    if (stream_bytes) *stream_bytes = fi.stream_bytes(precision);
    if (mfma_per_group) *mfma_per_group = fi.mfma_per_group(precision, h->cfg.framecode_ch > 0);
    return PG_OK;
}

int pg_stage_sample_coarse(pg_handle* h, void* stream, int64_t n, const float* ray_batch, const float* cyls,
                           int64_t cyl_stride, int n_samples, int flags, float* near_far, float* z) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n < 0 || !ray_batch || !cyls || !near_far || !z) return pg_fail(h, PG_EINVAL, "pg_stage_sample_coarse: null/negative argument");
    if (n_samples < 2) return pg_fail(h, PG_EINVAL, "pg_stage_sample_coarse: N_samples must be >= 2");
    PG_TRY(pg_check_cyl_stride(h, cyl_stride, true));
    PG_HIP(h, hipSetDevice(h->device));
    double* scs = nullptr;
    PG_TRY(pg_sc_scratch(h, n, h->cfg.chunk, &scs));
    PG_TRY_LAUNCH(h, "sample_coarse", pg_launch_sample_coarse(ray_batch, cyls, cyl_stride, n, h->cfg.chunk, n_samples,
                                                              (flags & PG_FLAG_LINDISP) ? 1 : 0, near_far, z, nullptr, scs, stream));
    return PG_OK;
}

int pg_stage_eval(pg_handle* h, void* stream, int which, int64_t n, int n_samples, const float* ray_batch,
                  const float* z, const float* skts, int64_t pose_stride, const float* cams, float* raw, float* dbg,
                  int dbg_stage) {
    PG_TRY(check_net(h, which, "pg_stage_eval"));
    if (n < 0 || !ray_batch || !z || !skts || !raw) return pg_fail(h, PG_EINVAL, "pg_stage_eval: null/negative argument");
    PG_TRY(pg_check_pose_stride(h, pose_stride, true));
    if (n == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    EvalCall c;
    c.which = which; c.n = n; c.S = n_samples; c.rays = ray_batch; c.z = z; c.skts = skts; c.pose_stride = pose_stride; c.cams = cams;
    c.raw = raw; c.dbg = dbg; c.dbg_stage = dbg_stage;
    c.colour_free = dbg && dbg_stage == 97;     // (a counting call runs as a render call's launch would: empty waves leave their colours out of `raw`)
    return launch_eval(h, stream, c);
}

int pg_query_density(pg_handle* h, void* stream, int which, int64_t n_points, const float* pts, const float* skts,
                     float* raw) {
    PG_TRY(check_net(h, which, "pg_query_density"));
    if (n_points < 0 || !pts || !skts || !raw) return pg_fail(h, PG_EINVAL, "pg_query_density: null/negative argument");
    if (n_points > 0x7fffffffLL) return pg_fail(h, PG_EINVAL, "pg_query_density: at most 2^31-1 points per call");
    if (n_points == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    // one pseudo ray (o = d = 0) that owns all points: the kernels take the pose and the view table
    // from the ray slot, the position from `pts`
    PG_TRY(ensure_ws(h, 256));
    PG_HIP(h, hipMemsetAsync(h->ws.p, 0, 64, static_cast<hipStream_t>(stream)));
    EvalCall c;
    c.which = which; c.n = 1; c.S = (int)n_points; c.rays = h->ws.as<const float>(); c.skts = skts; c.raw = raw; c.points = pts;
    return launch_eval(h, stream, c);
}

// The density grid of mesh extraction.  A grid row is a ray (pg_mesh.hip), so launch_eval picks the forms of a render call: the
// 16x16x32 kernel on chip or with records and pg_evalc2.hip from their sample minimum up, with limb masks.  Rows shorter than the picked
// form's minimum of samples per ray (or longer than the 256 samples the forms are measured and tested at) go as explicit points made on
// the device: the direct forms, as pg_query_density runs them.
int pg_grid_density(pg_handle* h, void* stream, int which, int res, double radius, const float* root, const float* skts,
                    int64_t slab_rays, float* sigma) {
    PG_TRY(check_net(h, which, "pg_grid_density"));
    if (!root || !skts || !sigma || slab_rays < 0) return pg_fail(h, PG_EINVAL, "pg_grid_density: null/negative argument");
    if (res < 1 || res > 1023) return pg_fail(h, PG_EINVAL, "pg_grid_density: res must be in [1, 1023], got %d", res);
    if (!(radius > 0.0) || !std::isfinite(radius)) return pg_fail(h, PG_EINVAL, "pg_grid_density: radius must be positive and finite");
    PG_HIP(h, hipSetDevice(h->device));
    const int R = res + 1;
    const long long rows_all = (long long)R * R;
    // t = np.linspace(-radius, radius, R).astype(float32): i * step + start in double, the last element the stop itself
    h->grid_t.resize(R);
    const double step = (radius - -radius) / res;
    for (int i = 0; i < R; ++i) { volatile double m = (double)i * step; h->grid_t[i] = (float)(m + -radius); }
    h->grid_t[R - 1] = (float)radius;
    const int prec = pass_precision(h->cfg.precision, false);
    const Form form = pick_form(CallFacts{prec, R, 0, h->cfg.framecode_ch > 0, false, false, false, 0, h->onchip_mode}, switches());
    const bool ray_form = R >= FORMS[form].points_per_pass() / (MAXR - 1) && R <= 256;
    // a slab's raw (16 B per point) stays within 256 MiB unless the caller sizes the slabs
    long long slab = slab_rays > 0 ? (long long)slab_rays : std::max(1ll, (256ll << 20) / (16ll * R));
    // Every slab starts on a pass boundary of every form (256 points): the limb masks are taken per pass and per wave, so only then
    // does a point share its pass with the same points as in one launch over the whole grid, and the slab size changes no value.
    long long align = 256;
    for (long long a = R, b = 256; b;) { const long long r = a % b; a = b; b = r; if (!b) align = 256 / a; }
    slab = std::max(align, slab / align * align);
    slab = std::min(slab, rows_all);
    float *d_t, *d_head, *d_in, *d_raw;
    PG_TRY(carve_ws(h, [&](Carver& c) {
        d_t = c.take<float>(R);
        d_head = c.take<float>(ray_form ? (size_t)slab * 11 : 64);                      // the slab's rays, or the one pseudo ray of the point form
        d_in = c.take<float>(ray_form ? (size_t)slab * R : (size_t)slab * R * 3);       // z [rows,R], or pts [rows R,3]
        d_raw = c.take<float>((size_t)slab * R * 4);
    }));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_HIP(h, hipMemcpyAsync(d_t, h->grid_t.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    if (!ray_form) PG_HIP(h, hipMemsetAsync(d_head, 0, 64, st));
    EvalCall ev;
    ev.which = which; ev.rays = d_head; ev.skts = skts; ev.raw = d_raw;
    for (long long r0 = 0; r0 < rows_all; r0 += slab) {
        const long long rows = std::min(slab, rows_all - r0);
        if (ray_form) {
            PG_TRY_LAUNCH(h, "grid setup kernel", pg_launch_grid_rays(root, d_t, R, r0, rows, d_head, d_in, stream));
            ev.n = rows; ev.S = R; ev.z = d_in;
        } else {
            PG_TRY_LAUNCH(h, "grid setup kernel", pg_launch_grid_points(root, d_t, R, r0 * R, rows * R, d_in, stream));
            ev.n = 1; ev.S = (int)(rows * R); ev.points = d_in;
        }
        PG_TRY(launch_eval(h, stream, ev));
        PG_TRY_LAUNCH(h, "density gather kernel", pg_launch_gather_sigma(d_raw, rows * R, sigma + r0 * R, stream));
    }
    return PG_OK;
}

int pg_stage_composite(pg_handle* h, void* stream, int64_t n, int n_samples, const float* ray_batch, const float* z,
                       const float* raw, float* rgb, float* disp, float* acc, float* alpha, float* weights,
                       int n_importance, float* z_fine) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n < 0 || !ray_batch || !z || !raw) return pg_fail(h, PG_EINVAL, "pg_stage_composite: null/negative argument");
    PG_TRY(check_samples(h, n_samples, n_importance, "pg_stage_composite: "));
    if (n_importance > 0 && n_samples < 3) return pg_fail(h, PG_EINVAL, "importance sampling needs N_samples >= 3");
    PG_HIP(h, hipSetDevice(h->device));
    pgk::Composite c{ray_batch, z, raw, n, n_samples, pgk::density_of(h->cfg), {rgb, disp, acc, alpha}};
    c.weights = weights; c.n_imp = n_importance; c.z_fine = z_fine;
    PG_TRY_LAUNCH(h, "composite", h->cfg.single_net ? pg_launch_composite_iso(&c, stream) : pg_launch_composite(&c, stream));
    return PG_OK;
}

int pg_stage_sample_coarse_draws(pg_handle* h, void* stream, int64_t n, const float* ray_batch, const float* cyls,
                                 int64_t cyl_stride, int n_samples, int flags, const float* t_rand, float* near_far, float* z) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n < 0 || !ray_batch || !cyls || !near_far || !z) return pg_fail(h, PG_EINVAL, "pg_stage_sample_coarse_draws: null/negative argument");
    if (n_samples < 2) return pg_fail(h, PG_EINVAL, "pg_stage_sample_coarse_draws: N_samples must be >= 2");
    PG_TRY(pg_check_cyl_stride(h, cyl_stride, true));
    PG_HIP(h, hipSetDevice(h->device));
    double* scs = nullptr;      // (without scratch the launcher runs the one-launch form at any chunk)
    if (!(flags & PG_FLAG_STAGE_ONE_LAUNCH)) PG_TRY(pg_sc_scratch(h, n, h->cfg.chunk, &scs));
    PG_TRY_LAUNCH(h, "sample_coarse", pg_launch_sample_coarse(ray_batch, cyls, cyl_stride, n, h->cfg.chunk, n_samples,
                                                              (flags & PG_FLAG_LINDISP) ? 1 : 0, near_far, z, t_rand, scs, stream));
    return PG_OK;
}

int pg_stage_composite_form(pg_handle* h, void* stream, int form, int64_t n, int n_samples, int n_importance, const float* ray_batch,
                            const float* z, const float* raw, const float* noise, const float* u_rand, float* rgb, float* disp,
                            float* acc, float* alpha, float* weights, float* z_fine, int32_t* order, float* z_new, int ld_new,
                            const float* raw_new, float* raw_out) {
    const char* fn = "pg_stage_composite_form";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (form != PG_COMP_PLAIN && form != PG_COMP_IS_ONLY && form != PG_COMP_MERGED) return pg_fail(h, PG_EINVAL, "%s: form %d is none of PG_COMP_*", fn, form);
    if (n < 0 || !ray_batch || !z || !raw) return pg_fail(h, PG_EINVAL, "%s: null/negative argument", fn);
    const int S = n_samples, N = n_importance;
    PG_TRY(check_samples(h, S, N, "pg_stage_composite_form: "));
    if (S + N > pg_composite_max_samples()) return pg_fail(h, PG_EINVAL, "%s: N_samples + N_importance exceeds %d", fn, pg_composite_max_samples());
    if (N > 0 && S < 3) return pg_fail(h, PG_EINVAL, "%s: importance sampling needs N_samples >= 3", fn);
    const bool merged = form == PG_COMP_MERGED;
    if (merged) {
        if (N < 2) return pg_fail(h, PG_EINVAL, "%s: the merged form needs N_importance >= 2", fn);
        if (!raw_new || !order) return pg_fail(h, PG_EINVAL, "%s: the merged form needs raw_new and order", fn);
        if (ld_new < N) return pg_fail(h, PG_EINVAL, "%s: ld_new %d < N_importance %d", fn, ld_new, N);
    } else {
        if (N > 0 && !z_fine) return pg_fail(h, PG_EINVAL, "%s: importance sampling needs z_fine", fn);
        if (form == PG_COMP_IS_ONLY && z_new && ld_new < N) return pg_fail(h, PG_EINVAL, "%s: ld_new %d < N_importance %d", fn, ld_new, N);
    }
    PG_HIP(h, hipSetDevice(h->device));
    // (the merged form composites the S + N sorted depths `z`; its launcher takes the total as S and the new ones as n_imp)
    pgk::Composite c{ray_batch, z, raw, n, merged ? S + N : S, pgk::density_of(h->cfg), {rgb, disp, acc, alpha}};
    c.noise = noise; c.n_imp = N; c.order = order;
    if (merged) {
        c.raw_new = raw_new; c.ld_new = ld_new; c.raw_out = raw_out;
        PG_TRY_LAUNCH(h, "composite", pg_launch_composite_merged(&c, stream));
        return PG_OK;
    }
    c.weights = weights; c.z_fine = z_fine; c.u_rand = u_rand;
    if (form == PG_COMP_IS_ONLY) { c.z_new = z_new; c.ld_new = ld_new; }
    PG_TRY_LAUNCH(h, "composite", form == PG_COMP_IS_ONLY ? pg_launch_composite_iso(&c, stream) : pg_launch_composite(&c, stream));
    return PG_OK;
}

namespace {

// one ray-level render call: the arguments of pg_render_rays / pg_render_rays_train
struct RayCall {
    int64_t n;
    const float *rays, *skts;
    int64_t pose_stride;
    const float* cyls;
    int64_t cyl_stride;
    const float* cams;
    int S, N, flags;
    const pg_train_draws* dr;       // null: eval mode
    const pg_outputs* out;
    bool rnoise() const { return dr && dr->ray_noise; }
    EvalCall eval(int which, int S_, const float* z, const float* pn, float* raw) const {   // a net on S_ samples per ray at the depths z
        EvalCall c;
        c.which = which; c.n = n; c.S = S_; c.rays = rays; c.z = z; c.skts = skts; c.pose_stride = pose_stride; c.cams = cams; c.raw = raw; c.pnoise = pn;
        return c;
    }
};

// The workspace of a render call, in the order it has always been carved (null: the call has no such buffer).  NP: the points per
// ray of single_net's second pass (0: the two-net pipeline)
struct RayBufs {
    float *nf, *zc, *rawc, *w0;     // near/far [n,2]; the coarse points' depths [n,S] and raw [n,S,4]; weights0 where the caller takes none
    float *zf, *rawf;               // merged depths [n,S+N]; two nets: the fine net's raw [n,S+N,4]
    int* order;                     // sort permutation of the merged depths [n,S+N]
    float *zn, *rawn;               // single_net: the new points' depths [n,NP] and raw [n,NP,4]
    float* pn;                      // position noise [.,3] of the pass being evaluated
    // A caller that takes the depths and the raw a pass works on (pg_outputs' z_coarse / raw_coarse / z_fine / raw_fine: tests, and
    // pg_render_scene, whose lists they are) gets them written in place, if its array is aligned like the workspace's (256 B): it
    // stands where the workspace's would.  Any other is filled by a copy at the end (copy_intermediates).
    int carve(pg_handle* h, const RayCall& r, int NP) {
        const size_t n = (size_t)r.n, S = r.S, SF = r.S + r.N;
        const bool hier = r.N > 0, single = NP > 0;
        const pg_outputs* o = r.out;
        auto in_place = [](float* p) { return p && !pg_misaligned(p, 256); };
        return carve_ws(h, [&](Carver& c) {
            nf = c.take<float>(n * 2);
            zc = in_place(o->z_coarse) ? o->z_coarse : c.take<float>(n * S);
            rawc = in_place(o->raw_coarse) ? o->raw_coarse : c.take<float>(n * S * 4);
            w0 = c.take<float>(n * S);
            zf = hier && in_place(o->z_fine) ? o->z_fine : c.take<float>(n * SF, hier);
            rawf = hier && !single && in_place(o->raw_fine) ? o->raw_fine : c.take<float>(n * SF * 4, hier && !single);
            order = c.take<int>(n * SF, single || (hier && r.rnoise()));
            zn = c.take<float>(n * NP, single);
            rawn = c.take<float>(n * NP * 4, single);
            pn = c.take<float>(n * (single ? std::max<size_t>(S, NP) : SF) * 3, r.rnoise());
        });
    }
};

// What both pipelines start with: near/far and the coarse depths -- with perturb the stratified jitter from the caller's draws
// (ray_utils.py:229-246) --, the position noise of the coarse points (rows [:S] of every ray's draws), net 0 on them, and their
// composite, which places the N importance depths: merged into b.zf and, single_net (NP > 0: the is_only pdf), in sample order
// into b.zn as well.  colour_free: skip_empty_ok.
int coarse_front(pg_handle* h, void* stream, const RayCall& r, const RayBufs& b, int NP, bool colour_free) {
    const pg_train_draws* dr = r.dr;
    const bool hier = r.N > 0, single = NP > 0;
    double* scs = nullptr;
    PG_TRY(pg_sc_scratch(h, r.n, h->cfg.chunk, &scs));
    PG_TRY_LAUNCH(h, "coarse sampling", pg_launch_sample_coarse(r.rays, r.cyls, r.cyl_stride, r.n, h->cfg.chunk, r.S, (r.flags & PG_FLAG_LINDISP) ? 1 : 0,
                                                                 b.nf, b.zc, dr ? dr->t_rand : nullptr, scs, stream));
    if (r.rnoise()) PG_TRY_LAUNCH(h, "noise gather", pg_launch_gather_noise(dr->ray_noise, r.n, r.S + r.N, r.S, nullptr, b.pn, stream));
    EvalCall ec = r.eval(0, r.S, b.zc, b.pn, b.rawc);
    ec.guide_pass = hier && !single;        // (single_net's coarse raw enters the fine maps: PG_PREC_FP16M runs it in fp16c)
    ec.colour_free = colour_free;
    PG_TRY(launch_eval(h, stream, ec));
    pgk::Composite cc{r.rays, b.zc, b.rawc, r.n, r.S, pgk::density_of(h->cfg), hier ? pgk::coarse_maps(*r.out) : pgk::final_maps(*r.out)};
    cc.noise = dr ? dr->noise0 : nullptr; cc.weights = r.out->weights0 ? r.out->weights0 : b.w0;
    cc.n_imp = r.N; cc.z_fine = b.zf; cc.u_rand = dr ? dr->u_rand : nullptr; cc.order = b.order; cc.z_new = b.zn; cc.ld_new = NP;
    PG_TRY_LAUNCH(h, "composite", single ? pg_launch_composite_iso(&cc, stream) : pg_launch_composite(&cc, stream));
    return PG_OK;
}

// and what both end with: the optional intermediates the caller asked for (raw_fine: null when a kernel has written it already)
int copy_intermediates(pg_handle* h, void* stream, const RayCall& r, const RayBufs& b, const float* raw_fine) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const pg_outputs* out = r.out;
    const size_t Pc = (size_t)r.n * r.S, Pf = (size_t)r.n * (r.S + r.N);
    if (out->near_far) PG_HIP(h, hipMemcpyAsync(out->near_far, b.nf, (size_t)r.n * 8, hipMemcpyDeviceToDevice, s));
    // (the depths and the raw were written in place, RayBufs::carve; single_net's merged raw is gathered into raw_fine by its composite)
    if (out->z_coarse && out->z_coarse != b.zc) PG_HIP(h, hipMemcpyAsync(out->z_coarse, b.zc, Pc * 4, hipMemcpyDeviceToDevice, s));
    if (out->raw_coarse && out->raw_coarse != b.rawc) PG_HIP(h, hipMemcpyAsync(out->raw_coarse, b.rawc, Pc * 16, hipMemcpyDeviceToDevice, s));
    if (r.N > 0 && out->z_fine && out->z_fine != b.zf) PG_HIP(h, hipMemcpyAsync(out->z_fine, b.zf, Pf * 4, hipMemcpyDeviceToDevice, s));
    if (raw_fine && out->raw_fine && out->raw_fine != raw_fine) PG_HIP(h, hipMemcpyAsync(out->raw_fine, raw_fine, Pf * 16, hipMemcpyDeviceToDevice, s));
    return PG_OK;
}

// single_net (core/raycasters.py:446-469): one net evaluates the S coarse points, then only the N new points drawn from the
// is_only pdf (sample_pts_is, is_only=True); the fine maps composite the S + N raw merged in depth order.  Arguments are
// checked by render_rays_impl.  S + N evaluations per ray instead of S + (S + N).
int render_rays_single(pg_handle* h, void* stream, const RayCall& r) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)r.n;
    const int S = r.S, N = r.N, SF = S + N;
    const pg_train_draws* dr = r.dr;
    const pg_outputs* out = r.out;
    // the new points are one pass of NP >= N points per ray: the direct 16-bit kernel needs points_per_pass / (MAXR - 1)
    // per ray (32); the columns behind N repeat the last new depth and are not read back
    const int prec = h->cfg.precision == PG_PREC_FP16M ? PG_PREC_FP16C : h->cfg.precision;
    const int NP = is_shape_a(prec) ? std::max(N, pg_eval16_points_per_pass() / (MAXR - 1)) : N;
    RayBufs b{};
    PG_TRY(b.carve(h, r, NP));
    // (the coarse raw is composited twice, by the coarse maps and merged into the fine ones: neither may draw density noise)
    PG_TRY(coarse_front(h, stream, r, b, NP, !out->raw_coarse && !out->raw_fine && !(dr && (dr->noise0 || dr->noise1))));
    if (r.rnoise()) {   // the new points' noise: rows [S:] in z_samples order (sample_pts_is, raycasters.py:665-674)
        int e = NP == N ? pg_launch_gather_noise(dr->ray_noise + (size_t)S * 3, r.n, SF, N, nullptr, b.pn, stream)
                        : (int)hipMemsetAsync(b.pn, 0, n * NP * 12, s);
        if (!e && NP != N)      // rows of NP: the N draws, then zeros for the padding points
            e = (int)hipMemcpy2DAsync(b.pn, (size_t)NP * 12, dr->ray_noise + (size_t)S * 3, (size_t)SF * 12, (size_t)N * 12, n,
                                      hipMemcpyDeviceToDevice, s);
        if (e) return pg_fail(h, PG_EHIP, "noise gather failed: %s", hipGetErrorString((hipError_t)e));
    }
    EvalCall en = r.eval(0, NP, b.zn, b.pn, b.rawn);
    en.colour_free = !out->raw_fine && !(dr && dr->noise1);
    PG_TRY(launch_eval(h, stream, en));
    pgk::Composite cm{r.rays, b.zf, b.rawc, r.n, SF, pgk::density_of(h->cfg), pgk::final_maps(*out)};
    cm.noise = dr ? dr->noise1 : nullptr; cm.n_imp = N; cm.order = b.order; cm.raw_new = b.rawn; cm.ld_new = NP; cm.raw_out = out->raw_fine;
    PG_TRY_LAUNCH(h, "composite", pg_launch_composite_merged(&cm, stream));
    return copy_intermediates(h, stream, r, b, nullptr);
}

int render_rays_impl(pg_handle* h, void* stream, const RayCall& r) {
    PG_TRY(check_ready(h, r.N > 0));
    if (r.n < 0 || !r.rays || !r.skts || !r.cyls || !r.out) return pg_fail(h, PG_EINVAL, "pg_render_rays: null/negative argument");
    PG_TRY(pg_check_pose_stride(h, r.pose_stride, false));
    PG_TRY(pg_check_cyl_stride(h, r.cyl_stride, false));
    PG_TRY(check_samples(h, r.S, r.N, ""));
    if (r.N > 0 && r.S + r.N > pg_composite_max_samples())
        return pg_fail(h, PG_EINVAL, "N_samples + N_importance exceeds %d", pg_composite_max_samples());
    if (r.n == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    if (h->cfg.single_net && r.N > 0) return render_rays_single(h, stream, r);
    const int SF = r.S + r.N;
    const pg_train_draws* dr = r.dr;
    const pg_outputs* out = r.out;
    RayBufs b{};
    PG_TRY(b.carve(h, r, 0));
    // what the empty-wave skip needs to know (skip_empty_ok): the launch's raw goes to one composite, without density noise, and to nobody else
    PG_TRY(coarse_front(h, stream, r, b, 0, !out->raw_coarse && !(dr && dr->noise0)));
    if (r.N > 0) {
        // every fine point keeps the noise of the stage it came from, in sorted order (raycasters.py:666-686)
        if (r.rnoise()) PG_TRY_LAUNCH(h, "noise gather", pg_launch_gather_noise(dr->ray_noise, r.n, SF, SF, b.order, b.pn, stream));
        EvalCall ef = r.eval(1, SF, b.zf, b.pn, b.rawf);
        ef.colour_free = !out->raw_fine && !(dr && dr->noise1);
        PG_TRY(launch_eval(h, stream, ef));
        pgk::Composite cf{r.rays, b.zf, b.rawf, r.n, SF, pgk::density_of(h->cfg), pgk::final_maps(*out)};
        cf.noise = dr ? dr->noise1 : nullptr;
        PG_TRY_LAUNCH(h, "composite", pg_launch_composite(&cf, stream));
    }
    return copy_intermediates(h, stream, r, b, b.rawf);
}
}  // namespace

int pg_render_rays(pg_handle* h, void* stream, int64_t n, const float* ray_batch, const float* skts,
                   int64_t pose_stride, const float* cyls, int64_t cyl_stride, const float* cams, int n_samples,
                   int n_importance, int flags, const pg_outputs* out) {
    return render_rays_impl(h, stream, RayCall{n, ray_batch, skts, pose_stride, cyls, cyl_stride, cams, n_samples, n_importance, flags, nullptr, out});
}

int pg_render_rays_train(pg_handle* h, void* stream, int64_t n, const float* ray_batch, const float* skts,
                         int64_t pose_stride, const float* cyls, int64_t cyl_stride, const float* cams, int n_samples,
                         int n_importance, int flags, const pg_train_draws* draws, const pg_outputs* out) {
    if (!draws) return pg_fail(h, PG_EINVAL, "pg_render_rays_train: null draws (use pg_render_rays for eval mode)");
    return render_rays_impl(h, stream, RayCall{n, ray_batch, skts, pose_stride, cyls, cyl_stride, cams, n_samples, n_importance, flags, draws, out});
}

int pg_pose_kinematics(pg_handle* h, void* stream, int64_t n_poses, const double* bones, const double* bone_offsets,
                       const int32_t* parents, float* kps, float* skts, double* l2ws) {
    const double* rest_pose = bone_offsets;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_poses < 0 || !bones || !rest_pose || !parents) return pg_fail(h, PG_EINVAL, "pg_pose_kinematics: null/negative argument");
    if (h->cfg.n_joints != 24) return pg_fail(h, PG_EINVAL, "pg_pose_kinematics: 24-joint SMPL skeleton only");
    pgkin::KinTree tree;
    int bad = 0;                        // the root's own entry is 0 here (the skeleton's table)
    if (parents[0] != 0 || !pgkin::pg_kin_tree(parents, tree, &bad))
        return pg_fail(h, PG_EINVAL, "pg_pose_kinematics: joint %d must come after its parent (%d)", bad, parents[bad]);
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY_LAUNCH(h, "pose kinematics kernel", pg_launch_pose_kinematics(rest_pose, &tree, bones, n_poses, kps, skts, l2ws, stream));
    return PG_OK;
}

int pg_pose_boxes(pg_handle* h, void* stream, int64_t n_poses, const float* kps, const double* w2c, int64_t w2c_stride,
                  const double* ring, double extension, double top_extension, double bot_extension, double fx, double fy,
                  int H, int W, int off_x, int off_y, float* cyls, int32_t* boxes) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_poses < 0 || !kps || !w2c || !ring || !cyls || !boxes || H <= 0 || W <= 0)
        return pg_fail(h, PG_EINVAL, "pg_pose_boxes: null/negative argument");
    if (w2c_stride != 0 && w2c_stride != 16) return pg_fail(h, PG_EINVAL, "pg_pose_boxes: w2c_stride must be 0 (one camera) or 16");
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY_LAUNCH(h, "pose box kernel", pg_launch_pose_boxes(kps, n_poses, w2c, w2c_stride, ring, (float)extension, (float)top_extension,
                                                             (float)bot_extension, fx, fy, H, W, off_x, off_y, cyls, boxes, stream));
    return PG_OK;
}

int pg_device_count(const pg_handle* h) { return h ? 1 + (int)h->peers.size() : 0; }

}  // extern "C"
