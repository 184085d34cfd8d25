// pg_scene.hip -- several posed people in one frame with mutual occlusion: pg_render_scene, pg_stage_scene_composite.
// Every person is rendered over its own box exactly as pg_render_frame renders it (pg_frames.h), except that what is kept per ray is
// not the maps but the list they are composited from: the depths z [S] and the raw [S,4].  All people share one camera, so the
// depths along a pixel's ray are comparable across people, and
//   scene_composite_kernel : one wave per pixel merges the lists of the people whose box holds the pixel by depth -- sample (q,k)
//                            precedes (p,i) if z_qk < z_pi, or z_qk == z_pi and (q,k) < (p,i) -- and composites the merged list with
//                            the lines of composite_ray (pg_kernels.hip).  Nothing is sorted: every list is non-decreasing already, so
//                            the transmittance in front of sample i of list p is p's own exclusive prefix product times, for every
//                            other list q, q's prefix product up to the number of q's samples that precede z_pi (a binary search).
//                            Pass 1, per list: sample s in lane s / E, E = ceil(S/64) (composite_ray's layout), exp in double, alpha
//                            and the factor from the one value, one wave_excl_scan_mul in double; the list's depths and its prefix
//                            table [S + 1] go to the wave's LDS rows.  Pass 2, per list: a sample's weight from its own entry and
//                            the other lists' looked-up entries, the weighted sums per lane, one wave reduction at the end (per
//                            person for person_acc).  Pass 2 forms alpha again from the depths in LDS and the raw in the cache: the
//                            same function on the same floats, so the same bits, and no per-list registers are kept across lists.
// LDS per wave and list: 257 doubles + 256 floats = 3080 B.  The kernel is instantiated for up to 2, 4 and 8 lists (PMAX) with 4, 4 and
// 2 waves per workgroup: 24.1 / 48.1 / 48.1 KB of static LDS, under 64 KB, and a scene of two people -- the common one -- runs at
// the occupancy its registers allow (5 waves per SIMD) instead of the 6 waves per CU that eight lists' rows would leave it.
// No atomics, lanes reduced by shuffles: two calls on the same inputs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pg_frame_dir.h"
#include "pg_frames.h"
#include "pg_handle.h"
#include "pg_launch.h"

namespace pgsc {

constexpr int MAXP = PG_SCENE_MAX_PEOPLE;
constexpr int MAXE = 4;                 // S <= 256 (CP_MAXS of pg_kernels.hip: pg_composite_max_samples)
constexpr int MAXS = 64 * MAXE;
constexpr int waves_for(int pmax) { return pmax <= 4 ? 4 : 2; }

struct Args {
    int P, S;
    pgk::Density den;
    const float* z[MAXP];               // [n_rows[p], S]
    const float4* raw[MAXP];            // [n_rows[p], S]
    long long n_rows[MAXP];
    long long npix;
    pgk::FrameGeom g;                   // FRAME: the camera; its box is the bounding rectangle of the people's boxes = the npix pixels
    int box[MAXP][4];                   // FRAME: (tlx, tly, bw, bh) of person p's clipped box; its row-major pixels are the rows of list p
    const int* rows;                    // stage: [P, npix] the row of pixel i in list p, outside [0, n_rows[p]): absent
    const float* dirs;                  // stage: [npix, 3] the pixels' ray directions
    float *rgb, *disp, *acc;            // [npix,3], [npix], [npix]
    float* pacc;                        // null, or FRAME: [P, H W] at the frame's pixel; stage: [P, npix]
};

// (see PG_WAVE_SYNC, pg_kernels.hip: LDS written by some lanes of a wave and read by others of the same wave)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the three wave primitives of composite_ray (pg_kernels.hip)
__device__ __forceinline__ double wave_excl_scan_mul(double x, int lane) {
    double incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(incl, off);
        if (lane >= off) incl *= t;
    }
    const double prev = __shfl_up(incl, 1);
    return lane == 0 ? 1.0 : prev;
}
template <typename V> __device__ __forceinline__ V wave_sum(V x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
// (a NaN comes out as NaN, as from F.relu / F.softplus: fmaxf would return its other operand)
__device__ __forceinline__ float density_act(float x, int act, float shift) {
    if (act == 0) return x < 0.0f ? 0.0f : x;
    const float t = x - shift;
    return t > 20.0f ? t : log1pf(expf(t));
}

// exp(-sigma delta) of one sample, composite_ray's lines: alpha = 1 - e and the factor e + 1e-10 both come from this value
__device__ __forceinline__ double sample_exp(float zs, float znext, bool last, float raw_w, float dnorm, const pgk::Density& den) {
    const float delta = (last ? 1e10f : znext - zs) * dnorm;
    const float sig = density_act(raw_w / den.scale, den.act, den.shift);
    return exp(-(double)(sig * delta));
}

// the row of pixel `pix` (FRAME: frame pixel (r, c)) in list p, or -1: person p does not cover it
template <bool FRAME>
__device__ __forceinline__ long long row_of(const Args& a, int p, long long pix, int r, int c) {
    if (FRAME) {
        const int x = c - a.box[p][0], y = r - a.box[p][1];
        return (x >= 0 && x < a.box[p][2] && y >= 0 && y < a.box[p][3]) ? (long long)y * a.box[p][2] + x : -1;
    }
    const long long row = a.rows[(long long)p * a.npix + pix];
    return (row >= 0 && row < a.n_rows[p]) ? row : -1;
}

// A wave takes pixels blockIdx.x * WAVES + wave, + gridDim.x * WAVES, ...  (a.P <= PMAX)
template <bool FRAME, int PMAX>
__global__ __launch_bounds__(waves_for(PMAX) * 64) void scene_composite_kernel(const Args a) {
    constexpr int WAVES = waves_for(PMAX);
    __shared__ double sh_pre[WAVES][PMAX][MAXS + 1];    // [list][s]: the product of the list's factors before sample s; [S]: of all
    __shared__ float sh_z[WAVES][PMAX][MAXS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.S, E = (S + 63) >> 6;
    for (long long pix = (long long)blockIdx.x * WAVES + wave; pix < a.npix; pix += (long long)gridDim.x * WAVES) {
        float d[3];
        int r = 0, c = 0;
        long long opix = pix;               // where person_acc holds this pixel
        if (FRAME) {
            r = a.g.tly + (int)(pix / a.g.bw); c = a.g.tlx + (int)(pix % a.g.bw);
            pgk::frame_ray_dir(a.g, r, c, d);
            opix = (long long)r * a.g.W + c;
        } else {
            d[0] = a.dirs[pix * 3]; d[1] = a.dirs[pix * 3 + 1]; d[2] = a.dirs[pix * 3 + 2];
        }
        const float dnorm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);     // (composite_ray's expression on the ray's d)
        const long long pacc_ld = FRAME ? (long long)a.g.H * a.g.W : a.npix;
        unsigned present = 0;
        for (int p = 0; p < a.P; ++p)
            if (row_of<FRAME>(a, p, pix, r, c) >= 0) present |= 1u << p;

        // ---- pass 1: every present list's depths and prefix table into the wave's LDS rows ----
        for (int p = 0; p < a.P; ++p) {
            if (!(present >> p & 1)) continue;
            const long long row = row_of<FRAME>(a, p, pix, r, c);
            const float* zr = a.z[p] + row * S;
            const float4* rr = a.raw[p] + row * S;
            double f_[MAXE];
            double lane_prod = 1.0;
#pragma unroll
            for (int e = 0; e < MAXE; ++e) {
                const int s = lane * E + e;
                f_[e] = 1.0;
                if (e < E && s < S) {
                    const float zs = zr[s];
                    const bool last = s + 1 >= S;
                    f_[e] = sample_exp(zs, last ? zs : zr[s + 1], last, rr[s].w, dnorm, a.den) + 1e-10;
                    sh_z[wave][p][s] = zs;
                    lane_prod *= f_[e];
                }
            }
            double T = wave_excl_scan_mul(lane_prod, lane);
#pragma unroll
            for (int e = 0; e < MAXE; ++e) {
                const int s = lane * E + e;
                if (e < E && s < S) {
                    sh_pre[wave][p][s] = T;
                    T *= f_[e];
                    if (s == S - 1) sh_pre[wave][p][S] = T;
                }
            }
        }
        wave_sync();

        // ---- pass 2: the weights in merged order, the sums ----
        float sr = 0, sg = 0, sb = 0, sd = 0;
        double swd = 0;
        for (int p = 0; p < a.P; ++p) {
            if (!(present >> p & 1)) {
                if (a.pacc && lane == 0) a.pacc[p * pacc_ld + opix] = 0.0f;
                continue;
            }
            const long long row = row_of<FRAME>(a, p, pix, r, c);
            const float4* rr = a.raw[p] + row * S;
            double swp = 0;
#pragma unroll
            for (int e = 0; e < MAXE; ++e) {
                const int s = lane * E + e;
                if (e < E && s < S) {
                    const float4 q4 = rr[s];
                    const float zs = sh_z[wave][p][s];
                    const bool last = s + 1 >= S;
                    const double ed = sample_exp(zs, last ? zs : sh_z[wave][p][s + 1], last, q4.w, dnorm, a.den);
                    const float alpha = (float)(1.0 - ed);
                    double T = sh_pre[wave][p][s];
                    for (int q = 0; q < a.P; ++q) {
                        if (q == p || !(present >> q & 1)) continue;
                        // the number of q's samples that precede (p, s): z_qk < z, or z_qk == z and q < p
                        const float* zq = sh_z[wave][q];
                        int lo = 0, hi = S;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            const float y = zq[mid];
                            if (y < zs || (q < p && y == zs)) lo = mid + 1; else hi = mid;
                        }
                        T *= sh_pre[wave][q][lo];
                    }
                    const float w = alpha * (float)T;
                    const float k = 1.0f + 2.0f * a.den.rgb_eps;
                    sr += w * ((1.0f / (1.0f + expf(-q4.x))) * k - a.den.rgb_eps);
                    sg += w * ((1.0f / (1.0f + expf(-q4.y))) * k - a.den.rgb_eps);
                    sb += w * ((1.0f / (1.0f + expf(-q4.z))) * k - a.den.rgb_eps);
                    sd += w * zs;
                    swp += (double)w;
                }
            }
            swd += swp;
            if (a.pacc) {
                const float pw = (float)wave_sum(swp);
                if (lane == 0) a.pacc[p * pacc_ld + opix] = pw > 1.0f ? 1.0f : pw;
            }
        }
        sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sd = wave_sum(sd);
        const float sw = (float)wave_sum(swd);
        if (lane == 0) {
            // (a pixel nobody covers: all sums are 0 -- disp 0 by the invalid mask below)
            a.rgb[pix * 3 + 0] = sr; a.rgb[pix * 3 + 1] = sg; a.rgb[pix * 3 + 2] = sb;
            // composite_ray's closing lines, comparisons instead of fmaxf / fminf: NaN sums give NaN maps, as torch.max / torch.minimum
            const float depth = sd / (sw + 1e-10f);
            float disp = 1.0f / (depth < 1e-10f ? 1e-10f : depth);
            if (fabsf(sw) <= 1e-8f) disp = 0.0f;        // torch.isclose(sum w, 0): |sum w| <= 1e-8
            a.disp[pix] = disp;
            a.acc[pix] = sw > 1.0f ? 1.0f : sw;
        }
        wave_sync();                        // the wave's LDS rows are reused by its next pixel
    }
}

template <bool FRAME, int PMAX>
int launch_for(const Args& a, int n_cu, void* stream) {
    constexpr int WAVES = waves_for(PMAX);
    const long long want = (a.npix + WAVES - 1) / WAVES;
    const int blocks = (int)std::min<long long>(want, (long long)std::max(n_cu, 1) * 32);
    hipLaunchKernelGGL((scene_composite_kernel<FRAME, PMAX>), dim3(blocks), dim3(WAVES * 64), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

template <bool FRAME>
int launch_form(const Args& a, int n_cu, void* stream) {
    if (a.P <= 2) return launch_for<FRAME, 2>(a, n_cu, stream);
    if (a.P <= 4) return launch_for<FRAME, 4>(a, n_cu, stream);
    return launch_for<FRAME, MAXP>(a, n_cu, stream);
}

int launch(const Args& a, bool frame, int n_cu, void* stream) {
    if (a.npix <= 0 || a.P < 1 || a.P > MAXP) return 0;
    return frame ? launch_form<true>(a, n_cu, stream) : launch_form<false>(a, n_cu, stream);
}

// What a handle keeps between pg_render_scene calls, grow-only: the people's lists (20 B per sample) and the maps of the bounding
// rectangle (20 B per pixel).
struct SceneState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_SCENE;
    ~SceneState() override { pg_release(lists); pg_release(maps); }
    DevBuf lists, maps;
};

}  // namespace pgsc

extern "C" {

int pg_render_scene(pg_handle* h, void* stream, int H, int W, const float* c2w, const float* intrinsics, float near, float far,
                    int n_people, const pg_scene_person* people, int n_samples, int n_importance, int flags, const float* bg,
                    float base_bg, float* rgb, float* disp, float* acc, uint8_t* rgb8, float* person_acc, float* const* lists) {
    using namespace pgsc;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!people || !rgb || H <= 0 || W <= 0 || !c2w || !intrinsics) return pg_fail(h, PG_EINVAL, "pg_render_scene: null/non-positive argument");
    if (n_people < 1 || n_people > MAXP) return pg_fail(h, PG_EINVAL, "pg_render_scene: %d people (1..%d)", n_people, MAXP);
    if (!h->peers.empty()) return pg_fail(h, PG_EINVAL, "pg_render_scene: a handle on several devices (scenes render on one)");
    if (h->tape_out) return pg_fail(h, PG_EINVAL, "pg_render_scene: a training tape is outstanding (run its backward first)");
    const int SF = n_samples + (n_importance > 0 ? n_importance : 0);
    if (n_samples < 1 || n_importance < 0 || SF > MAXS) return pg_fail(h, PG_EINVAL, "pg_render_scene: N_samples + N_importance = %d outside [1, %d]", SF, MAXS);
    Args a{};
    a.P = n_people; a.S = SF; a.den = pgk::density_of(h->cfg);
    pgk::FrameGeom gp[MAXP];
    int x0 = W, y0 = H, x1 = 0, y1 = 0;
    for (int p = 0; p < n_people; ++p) {
        const pg_scene_person& q = people[p];
        if (q.subject < 0 || q.subject >= bank_count(h->bank))
            return pg_fail(h, PG_EINVAL, "pg_render_scene: person %d names subject %d of %d", p, q.subject, bank_count(h->bank));
        if (!q.skts || !q.cyl) return pg_fail(h, PG_EINVAL, "pg_render_scene: person %d without skts / cyl", p);
        PG_TRY(frame_geom(h, H, W, c2w, intrinsics, q.box, near, far, q.cam, &gp[p]));
        const pgk::FrameGeom& g = gp[p];
        a.box[p][0] = g.tlx; a.box[p][1] = g.tly; a.box[p][2] = g.bw; a.box[p][3] = g.bh;
        a.n_rows[p] = (long long)g.bw * g.bh;
        if (a.n_rows[p] == 0) { a.box[p][2] = a.box[p][3] = 0; continue; }
        x0 = std::min(x0, g.tlx); y0 = std::min(y0, g.tly); x1 = std::max(x1, g.tlx + g.bw); y1 = std::max(y1, g.tly + g.bh);
    }
    // the bounding rectangle of the boxes: the pixels the kernel writes, and the box frame_compose scatters
    a.g = gp[0];
    a.g.tlx = x1 > x0 ? x0 : 0; a.g.tly = y1 > y0 ? y0 : 0;
    a.g.bw = x1 > x0 ? x1 - x0 : 0; a.g.bh = y1 > y0 ? y1 - y0 : 0;
    a.npix = (long long)a.g.bw * a.g.bh;
    PG_HIP(h, hipSetDevice(h->device));
    SceneState* stp = nullptr;
    PG_TRY(pg_state(h, stp));
    SceneState& st = *stp;
    float* zs[MAXP];
    float* raws[MAXP];
    auto carve_lists = [&](Carver& c) {
        for (int p = 0; p < n_people; ++p) {
            zs[p] = c.take<float>((size_t)a.n_rows[p] * SF);
            raws[p] = c.take<float>((size_t)a.n_rows[p] * SF * 4);
        }
    };
    FrameMaps maps{};
    auto carve_maps = [&](Carver& c) {
        maps.rgb_map = c.take<float>((size_t)a.npix * 3);
        maps.disp_map = c.take<float>((size_t)a.npix);
        maps.acc_map = c.take<float>((size_t)a.npix);
    };
    Carver sl, sm;
    carve_lists(sl);
    carve_maps(sm);
    PG_TRY(pg_grow(h, st.lists, sl.off, "scene sample lists", sl.off + sl.off / 8));
    PG_TRY(pg_grow(h, st.maps, sm.off, "scene maps", sm.off + sm.off / 8));
    Carver cl{st.lists.p}, cm{st.maps.p};
    carve_lists(cl);
    carve_maps(cm);
    // every person over its own box, as pg_render_frame renders it (its maps are not wanted: null), with its subject selected -- a
    // pointer swap between two enqueues -- and the selection put back
    const int active0 = h->bank.active;
    const FrameMaps none{nullptr, nullptr, nullptr};
    int rc = PG_OK;
    for (int p = 0; p < n_people && rc == PG_OK; ++p) {
        a.z[p] = zs[p]; a.raw[p] = reinterpret_cast<const float4*>(raws[p]);
        bank_select(*h, h->bank, people[p].subject);
        const FrameLists fl{zs[p], raws[p]};
        rc = frame_render_range(h, stream, gp[p], 0, a.n_rows[p], people[p].skts, people[p].cyl, n_samples, n_importance, flags, nullptr, &none, &fl);
    }
    bank_select(*h, h->bank, active0);
    PG_TRY(rc);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lists)
        for (int p = 0; p < n_people; ++p) {
            const size_t n = (size_t)a.n_rows[p] * SF;
            if (n && lists[2 * p]) PG_HIP(h, hipMemcpyAsync(lists[2 * p], zs[p], n * 4, hipMemcpyDeviceToDevice, s));
            if (n && lists[2 * p + 1]) PG_HIP(h, hipMemcpyAsync(lists[2 * p + 1], raws[p], n * 16, hipMemcpyDeviceToDevice, s));
        }
    a.rgb = maps.rgb_map; a.disp = maps.disp_map; a.acc = maps.acc_map;
    a.pacc = person_acc;
    if (person_acc) PG_HIP(h, hipMemsetAsync(person_acc, 0, (size_t)n_people * H * W * sizeof(float), s));
    PG_TRY_LAUNCH(h, "scene composite kernel", launch(a, true, h->n_cu, stream));
    return frame_compose(h, stream, a.g, maps, bg, base_bg, rgb, disp, acc, rgb8);
}

int pg_stage_scene_composite(pg_handle* h, void* stream, int64_t n_pix, int n_people, int n_samples, const float* const* z,
                             const float* const* raw, const int64_t* n_rows, const int32_t* rows, const float* dirs, float* rgb,
                             float* disp, float* acc, float* person_acc) {
    using namespace pgsc;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_pix < 0 || !z || !raw || !n_rows || !rows || !dirs || !rgb || !disp || !acc) return pg_fail(h, PG_EINVAL, "pg_stage_scene_composite: null/negative argument");
    if (n_people < 1 || n_people > MAXP) return pg_fail(h, PG_EINVAL, "pg_stage_scene_composite: %d people (1..%d)", n_people, MAXP);
    if (n_samples < 1 || n_samples > MAXS) return pg_fail(h, PG_EINVAL, "pg_stage_scene_composite: %d samples per list (1..%d)", n_samples, MAXS);
    Args a{};
    a.P = n_people; a.S = n_samples; a.den = pgk::density_of(h->cfg);
    for (int p = 0; p < n_people; ++p) {
        if (n_rows[p] < 0 || (n_rows[p] > 0 && (!z[p] || !raw[p]))) return pg_fail(h, PG_EINVAL, "pg_stage_scene_composite: list %d is null or of negative length", p);
        if (pg_misaligned(raw[p], 16)) return pg_fail(h, PG_EINVAL, "pg_stage_scene_composite: raw of list %d is not 16-byte aligned", p);
        a.z[p] = z[p]; a.raw[p] = reinterpret_cast<const float4*>(raw[p]); a.n_rows[p] = n_rows[p];
    }
    a.npix = n_pix; a.rows = rows; a.dirs = dirs;
    a.rgb = rgb; a.disp = disp; a.acc = acc; a.pacc = person_acc;
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY_LAUNCH(h, "scene composite kernel", launch(a, false, h->n_cu, stream));
    return PG_OK;
}

}  // extern "C"
