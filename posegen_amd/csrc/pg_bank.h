// pg_bank.h -- the subject bank of a renderer handle: S >= 1 complete models ("subjects": independent checkpoints of one
// architecture) behind one pg_handle.  Host-only and free of HIP calls, so that the swap logic compiles into a plain C++ program
// (tools/sanitize/subject_bank_asan.cpp, built with the address and undefined-behaviour sanitisers); device memory is allocated and
// released through the caller's functors.
//
// What a subject owns is `Subject`: both nets' NetState (host tensors, folded view layer, every packed image, source maps, frame
// codes, the widened view weight), the embedder's cutoffs and taus, and a device copy of the cutoffs OF ITS OWN.  A launch reads
// the cutoffs through a pointer: one buffer rewritten per selection would change under a launch still in flight.
// Everything else on the handle is shared: configuration, precision, workspaces, record buffers, frame caches, streams.
//
// The handle IS the active subject (pg_handle derives from Subject: h->net, h->cut, ... are the active model's, as before there was
// a bank).  The other subjects wait in Bank::parked; parked[active] is hollow.  bank_select swaps: NetState moves by pointer and
// vector swaps, no allocation, no copy, nothing on the device.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/posegen_hip.h"

// The packed weight images of one net.  pg_api.hip packs and uploads one on first use (ensure_image) and says which of them a
// form of the fused kernel reads (FORMS).  The first four kinds exist per kernel arithmetic: id = kind + PG_PREC_*.
enum Image : int {
    IMG_NONE = -1,
    IMG_DIRECT = 0,                                 // stream of the direct-view kernels: pg_eval16.hip (bf16 / fp16, shape A), pg_eval32.hip (the others, k-major shape B)
    IMG_REC16 = IMG_DIRECT + PG_PREC_COUNT,         // 16x16x32 kernel with per-ray records (pg_eval16r.hip): stream
    IMG_ONCHIP16 = IMG_REC16 + PG_PREC_COUNT,       // ... its on-chip variant (no per-ray records): stream
    IMG_VY16 = IMG_ONCHIP16 + PG_PREC_COUNT,        // Y-stage weights of the per-ray record kernel (pg_rayrec.hip)
    IMG_PER_PREC_END = IMG_VY16 + PG_PREC_COUNT,
    IMG_C2 = IMG_PER_PREC_END,                      // compensated-fp16 kernel with the out tiles over the waves (pg_evalc2.hip): weights (pg_program.h T)
    IMG_YCODE,                                      // on-chip 16x16x32 variant with frame codes: Yc[n_codes + 1][128] = W_view[:, 904:920] codes[c]
    IMG_BIAS16,                                     // 16-row bias table (the 16x16x32 kernel, pg_evalc2.hip)
    IMG_BIAS,                                       // 32-row bias table (every other kernel)
    IMG_COUNT
};
enum SrcMap : int { MAP_NONE = -1, MAP_ONCHIP16 = 0 /* one map for bf16 and fp16 */, MAP_C2, MAP_BIAS16, MAP_COUNT };

struct NetState {
    bool loaded = false;
    std::vector<std::vector<float>> host;      // 24 tensors, reference order (see header)
    std::vector<float> codes_host;             // [n_codes+1,16]
    mutable std::vector<float> fold_w, fold_b; // W_view[:, :256] W_feature and its bias (NetTensors::fold), formed once per pg_load_weights
    int n_codes = 0;
    struct Slot { uint8_t* d = nullptr; size_t bytes = 0; } img[IMG_COUNT];
    float* d_codes = nullptr;
    // pg_load_weights_device: the net's tensors as one flat device vector (NetTensors::layout; + the folded view layer), the
    // source maps of the images that are re-formed by a gather, and whether `host` lags the device copy
    float* d_src = nullptr;
    int32_t* d_map[MAP_COUNT] = {};
    float* d_vwide = nullptr;      // multires_views = 0: the caller's view weight widened to the 4-band layout (pg_launch_widen_views)
    bool host_stale = false;
    int64_t builds = 0;            // images built so far: ensure_image packs + device re-forms (pg_subject_info)
};

// One model of the bank
struct Subject {
    NetState net[2];
    float cut[48] = {};
    float tau[2] = {20.f, 20.f};
    bool emb_set[2] = {false, false};
    float* d_cut = nullptr;        // the cutoffs on the device, one buffer PER SUBJECT (see above)
};

struct Bank {
    std::vector<Subject> parked;   // [n_subjects] once there is more than one subject (empty: a one-subject handle)
    int active = 0;
};

inline int bank_count(const Bank& b) { return b.parked.empty() ? 1 : (int)b.parked.size(); }

inline void subject_swap(Subject& a, Subject& b) {
    for (int w = 0; w < 2; ++w) std::swap(a.net[w], b.net[w]);
    std::swap(a.cut, b.cut);
    std::swap(a.tau, b.tau);
    std::swap(a.emb_set, b.emb_set);
    std::swap(a.d_cut, b.d_cut);
}

// Subject s becomes the active one (`act`: the handle's own Subject part).  The caller has checked the range.
inline void bank_select(Subject& act, Bank& b, int s) {
    if (s == b.active) return;
    subject_swap(act, b.parked[b.active]);     // the active model goes to its own place, which was hollow ...
    subject_swap(act, b.parked[s]);            // ... and subject s comes out of its place, which is hollow now
    b.active = s;
}

// n subjects.  Growing keeps every subject and readies the new ones with `make(Subject&) -> int` (0 = ok; it allocates the
// subject's d_cut and fills its cutoffs); shrinking hands the dropped ones to `drop(Subject&)`, which frees what they hold on the
// device.  The active subject must be one that stays (the caller refuses otherwise).  Returns `make`'s first failure, with the bank
// at the size reached.
template <class Make, class Drop>
int bank_resize(Subject& act, Bank& b, int n, Make&& make, Drop&& drop) {
    (void)act;
    const int have = bank_count(b);
    if (n == have) return 0;
    if (n < have) {
        for (int s = n; s < have; ++s) drop(b.parked[s]);
        if (n == 1) { b.parked.clear(); b.parked.shrink_to_fit(); }
        else b.parked.resize((size_t)n);
        return 0;
    }
    if (b.parked.empty()) b.parked.resize(1);  // (the hollow place of subject 0, the active one)
    b.parked.reserve((size_t)n);
    for (int s = have; s < n; ++s) {
        b.parked.emplace_back();
        if (const int rc = make(b.parked.back())) { drop(b.parked.back()); b.parked.pop_back(); if (b.parked.size() == 1) b.parked.clear(); return rc; }
    }
    return 0;
}
