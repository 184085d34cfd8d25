// pg_metrics.hip -- a rendered frame scored against its ground truth on the device: the sums behind the PSNR, the SSIM
// and their foreground-masked variants of the reference's two evaluate_metric functions (run_render.py:888-974,
// core/utils/evaluation_helpers.py:257-385), over a 2-D box of the frame.
//   frame_metrics_kernel     : one workgroup per tile of 32 x 32 SSIM-map pixels.  The tile's 42 x 42 box pixels (a 10-pixel halo: the
//                              11 x 11 window, valid convolution) of the frame, the ground truth (bytes / 255, the background's byte where
//                              the mask is 0 with PG_METRICS_BG) and the mask are staged into LDS once; the squared errors of the
//                              pixels the tile owns are added while they pass.  Then per channel: the five window moments (x, y, x^2,
//                              y^2, xy) along rows into LDS, along columns out of it, pytorch_msssim's ssim_map formula, and the sums
//                              of the map and of the map under the mask at the window's centre.  The map is never written.  The
//                              tile's eight partial sums go to its own slot.
//   frame_metrics_sum_kernel : the slots added in tile index order: sums[8].
// pg_frame_metrics_val runs the same kernel with two compile-time switches.  UP: the frame is given at h x w <= H x W
// and the staged frame value is its bilinear upsampling (F.interpolate, align_corners = False, index arithmetic in double) -- a tile
// fills the taps of its <= 42 staged rows and columns into LDS, a staging lane blends its four texels in double and stores the
// float32.  VALID: four more sums over a second rectangle of the frame (a box pixel inside it; a map pixel whose window centre is),
// 12 doubles per slot.  Everything behind staging is the same code, <false, false> is pg_frame_metrics.
// Every sum, window sum and the map's arithmetic is double (the variance is a cancellation; 0.5 GFLOP per 1000 x 1000 frame).  No
// atomics: lanes are reduced by shuffles, waves and tiles in index order, so two calls on the same inputs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_handle.h"
#include "pg_metrics_plan.h"

namespace pgs {

using namespace pgsp;

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int PLANE = STAGE * STAGE;         // one channel of the staged tile, [row][col]: lanes walk col, any row stride is conflict-free
constexpr int HROWS = STAGE * TILE;          // one moment after the row pass, [row][map col] doubles
constexpr double C1 = 1e-4, C2 = 9e-4;       // (0.01 L)^2, (0.03 L)^2 with L = 1

struct Args {
    const float* rgb;        // [H,W,3] the rendered frame
    const uint8_t* img;      // [P,3] the image's row of the bank
    const uint8_t* mask;     // [P] or null: no foreground
    const uint8_t* bg;       // [P,3] the image's background, or null: gt = img
    int W;
    int x0, y0, w, h;        // the box
    int ntx;
    double taps[WIN];
    double* slots;
    int H, lh, lw;           // UP: the frame's height; rgb is [lh,lw,3]
    int vx0, vy0, vx1, vy1;  // VALID: the valid rectangle relative to the box's corner (it may reach outside the box)
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// ssim_map of pytorch_msssim.ssim at one pixel from the five window means.  Nothing is contracted: with x == y the numerator and the
// denominator are the same operations on the same numbers and the value is exactly 1.
__device__ __forceinline__ double ssim_value(double ex, double ey, double exx, double eyy, double exy) {
#pragma clang fp contract(off)
    const double mu1_sq = ex * ex, mu2_sq = ey * ey, mu1_mu2 = ex * ey;
    const double sigma1_sq = exx - mu1_sq, sigma2_sq = eyy - mu2_sq, sigma12 = exy - mu1_mu2;
    const double v1 = 2.0 * sigma12 + C2;
    const double v2 = sigma1_sq + sigma2_sq + C2;
    return ((2.0 * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2);
}

template <bool UP, bool VALID>
__global__ __launch_bounds__(THREADS) void frame_metrics_kernel(Args a) {
    __shared__ float sx[3 * PLANE], sy[3 * PLANE];       // frame and ground truth, [channel][row][col]
    __shared__ double hm[5 * HROWS];                     // the row pass of one channel, [moment][row][map col]
    __shared__ uint8_t sm[PLANE];                        // mask > 0
    __shared__ double red[WAVES][VALID ? 6 : 4];
    __shared__ Tap tab[UP ? 2 * STAGE : 1];              // UP: the taps of the staged rows, then of the staged columns
    __shared__ int redi[WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx = blockIdx.x % a.ntx, ty = blockIdx.x / a.ntx;
    const Span xs = tile_span(a.w, tx), ys = tile_span(a.h, ty);

    if constexpr (UP) {
        for (int k = tid; k < 2 * STAGE; k += THREADS) {
            const int i = k < STAGE ? k : k - STAGE;
            if (k < STAGE) { if (i < ys.sn) tab[k] = resample_tap(a.lh, a.H, a.y0 + ys.s0 + i); }
            else if (i < xs.sn) tab[k] = resample_tap(a.lw, a.W, a.x0 + xs.s0 + i);
        }
        __syncthreads();
    }

    // stage: a wave per row, a lane per (col, channel) -- the row's 3 sn consecutive floats / bytes of the frame and the image
    double se = 0.0, se_fg = 0.0, ssim = 0.0, ssim_fg = 0.0;
    [[maybe_unused]] double se_val = 0.0, ssim_val = 0.0;
    int n_fg = 0, n_fg_map = 0;
    for (int r = wv; r < STAGE; r += WAVES) {
        const long long prow = (long long)(a.y0 + ys.s0 + r) * a.W + (a.x0 + xs.s0);
        for (int k = lane; k < STAGE * 3; k += 64) {
            const int col = k / 3, ch = k - col * 3;
            float xv = 0.0f, yv = 0.0f;
            bool m = false;
            if (r < ys.sn && col < xs.sn) {
                const long long p = prow + col;
                if constexpr (UP) {
                    const Tap tr = tab[r], tc = tab[STAGE + col];
                    const float* r0 = a.rgb + (size_t)tr.i0 * a.lw * 3 + ch;
                    const float* r1 = a.rgb + (size_t)tr.i1 * a.lw * 3 + ch;
                    xv = resample_blend((double)r0[tc.i0 * 3], (double)r0[tc.i1 * 3], (double)r1[tc.i0 * 3], (double)r1[tc.i1 * 3], tc.l1, tr.l1);
                } else {
                    xv = a.rgb[p * 3 + ch];
                }
                m = a.mask && a.mask[p] > 0;
                uint8_t b = a.img[p * 3 + ch];
                if (a.bg && !m) b = a.bg[p * 3 + ch];
                yv = __fdiv_rn((float)b, 255.0f);
                if (r < ys.own && col < xs.own) {
                    const double d = (double)yv - (double)xv;
                    se += d * d;
                    if (m) { se_fg += d * d; ++n_fg; }
                    if constexpr (VALID) {
                        const int bx = xs.s0 + col, by = ys.s0 + r;
                        if (bx >= a.vx0 && bx < a.vx1 && by >= a.vy0 && by < a.vy1) se_val += d * d;
                    }
                }
            }
            sx[ch * PLANE + r * STAGE + col] = xv;
            sy[ch * PLANE + r * STAGE + col] = yv;
            if (ch == 0) sm[r * STAGE + col] = m ? 1 : 0;
        }
    }
    __syncthreads();

    if (xs.map > 0 && ys.map > 0) {
        for (int ch = 0; ch < 3; ++ch) {
            // along rows: staged row r, map column c <- the window over staged columns [c, c + WIN)
            for (int idx = tid; idx < HROWS; idx += THREADS) {
                const int r = idx / TILE, c = idx % TILE;
                const float* px = sx + ch * PLANE + r * STAGE + c;
                const float* py = sy + ch * PLANE + r * STAGE + c;
                double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
                for (int t = 0; t < WIN; ++t) {
                    const double x = (double)px[t], y = (double)py[t], g = a.taps[t];
                    const double gx = g * x, gy = g * y;
                    hx += gx; hy += gy; hxx += gx * x; hyy += gy * y; hxy += gx * y;
                }
                hm[0 * HROWS + idx] = hx; hm[1 * HROWS + idx] = hy; hm[2 * HROWS + idx] = hxx; hm[3 * HROWS + idx] = hyy; hm[4 * HROWS + idx] = hxy;
            }
            __syncthreads();
            // along columns: map pixel (i, j) <- rows [i, i + WIN) of column j
            for (int idx = tid; idx < TILE * TILE; idx += THREADS) {
                const int i = idx / TILE, j = idx % TILE;
                const double* ph = hm + i * TILE + j;
                double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < WIN; ++t) {
                    const double g = a.taps[t];
#pragma unroll
                    for (int q = 0; q < 5; ++q) e[q] += g * ph[q * HROWS + t * TILE];
                }
                if (i < ys.map && j < xs.map) {
                    const double v = ssim_value(e[0], e[1], e[2], e[3], e[4]);
                    ssim += v;
                    if (sm[(i + WIN / 2) * STAGE + j + WIN / 2]) { ssim_fg += v; ++n_fg_map; }
                    if constexpr (VALID) {
                        const int bx = xs.s0 + j + WIN / 2, by = ys.s0 + i + WIN / 2;
                        if (bx >= a.vx0 && bx < a.vx1 && by >= a.vy0 && by < a.vy1) ssim_val += v;
                    }
                }
            }
            __syncthreads();
        }
    }

    // lanes by shuffles, then the waves in index order
    se = wave_sum(se); se_fg = wave_sum(se_fg); ssim = wave_sum(ssim); ssim_fg = wave_sum(ssim_fg);
    n_fg = wave_sum(n_fg); n_fg_map = wave_sum(n_fg_map);
    if constexpr (VALID) { se_val = wave_sum(se_val); ssim_val = wave_sum(ssim_val); }
    if (lane == 0) {
        red[wv][0] = se; red[wv][1] = se_fg; red[wv][2] = ssim; red[wv][3] = ssim_fg;
        redi[wv][0] = n_fg; redi[wv][1] = n_fg_map;
        if constexpr (VALID) { red[wv][4] = se_val; red[wv][5] = ssim_val; }
    }
    __syncthreads();
    if (tid == 0) {
        constexpr int NR = VALID ? 6 : 4;
        double s[NR] = {};
        int c[2] = {0, 0};
        for (int w = 0; w < WAVES; ++w) {
            for (int q = 0; q < NR; ++q) s[q] += red[w][q];
            c[0] += redi[w][0]; c[1] += redi[w][1];
        }
        double* o = a.slots + slot_offset(a.ntx, tx, ty, VALID ? SUMS_VAL : SUMS);
        o[0] = 3.0 * xs.own * ys.own; o[1] = s[0]; o[2] = (double)c[0]; o[3] = s[1];     // (n_fg: a lane per channel has counted 3 m)
        o[4] = 3.0 * xs.map * ys.map; o[5] = s[2]; o[6] = (double)c[1]; o[7] = s[3];
        if constexpr (VALID) {
            // the counts from the spans: own pixels inside the rectangle, map pixels whose window centre is
            const bool has_map = xs.map > 0 && ys.map > 0;
            o[8] = 3.0 * overlap(xs.s0, xs.s0 + xs.own, a.vx0, a.vx1) * overlap(ys.s0, ys.s0 + ys.own, a.vy0, a.vy1);
            o[9] = s[4];
            o[10] = has_map ? 3.0 * overlap(xs.s0 + WIN / 2, xs.s0 + WIN / 2 + xs.map, a.vx0, a.vx1) *
                                  overlap(ys.s0 + WIN / 2, ys.s0 + WIN / 2 + ys.map, a.vy0, a.vy1) : 0.0;
            o[11] = s[5];
        }
    }
}

// sums[c] = slots[0][c] + slots[1][c] + ... in this order, a lane per sum; N doubles per slot, sums[N .. OUT) = 0
template <int N, int OUT>
__global__ __launch_bounds__(64) void frame_metrics_sum_kernel(const double* __restrict__ slots, int ntiles, double* __restrict__ sums) {
    const int c = threadIdx.x;
    if (c >= OUT) return;
    double acc = 0.0;
    if (c < N) {
#pragma unroll 8
        for (int t = 0; t < ntiles; ++t) acc += slots[(size_t)t * N + c];
    }
    sums[c] = acc;
}

}  // namespace pgs

// ---- the host side: the entry point of the C ABI and what it keeps in the handle ------------------------------------------------------
namespace {

// the tiles' partial sums.  One buffer per handle: calls on one handle are serialised by the caller, and calls enqueued on different
// streams have to be ordered by the caller as well.
struct MetricsState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_METRICS;
    ~MetricsState() override { pg_release(slots); }
    DevBuf slots;
};

template <bool UP, bool VALID>
void launch_tiles(const pgs::Args& a, int ntiles, hipStream_t st) {
    hipLaunchKernelGGL((pgs::frame_metrics_kernel<UP, VALID>), dim3((unsigned)ntiles), dim3(pgs::THREADS), 0, st, a);
}

// Both entry points: the checks, then the tile kernel and the ordered sum.  `wide`: pg_frame_metrics_val -- rgb is [rgb_h,rgb_w,3],
// `valid` may be null, sums has 12 entries.
int frame_metrics(pg_handle* h, const char* who, bool wide, void* stream, const pg_image_bank* bank, int32_t img_row, const int32_t box[4],
                  const float* rgb, int32_t rgb_h, int32_t rgb_w, const int32_t* valid, int flags, double* sums) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!bank || !box || !rgb || !sums) return pg_fail(h, PG_EINVAL, "%s: null argument", who);
    if (flags & ~PG_METRICS_BG) return pg_fail(h, PG_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (!bank->imgs) return pg_fail(h, PG_EINVAL, "%s: the bank's imgs are required", who);
    if (bank->F <= 0 || bank->P <= 0) return pg_fail(h, PG_EINVAL, "%s: F and P must be positive", who);
    if (bank->H <= 0 || bank->W <= 0 || (int64_t)bank->H * bank->W != bank->P || bank->P > 0x7ffffffell)
        return pg_fail(h, PG_EINVAL, "%s: H x W = %d x %d is not P = %lld", who, bank->H, bank->W, (long long)bank->P);
    if (img_row < 0 || img_row >= bank->F) return pg_fail(h, PG_EINVAL, "%s: img_row = %d is outside [0, %lld)", who, img_row, (long long)bank->F);
    if (!pgsp::box_ok(box, bank->H, bank->W))
        return pg_fail(h, PG_EINVAL, "%s: box (%d, %d, %d, %d) is empty or outside the %d x %d frame", who, box[0], box[1], box[2], box[3], bank->H, bank->W);
    if (wide) {
        if (rgb_h < 1 || rgb_w < 1 || rgb_h > bank->H || rgb_w > bank->W)
            return pg_fail(h, PG_EINVAL, "%s: a frame of %d x %d against %d x %d images (1 <= rgb_h <= H, 1 <= rgb_w <= W; there is no downsampling)",
                           who, rgb_h, rgb_w, bank->H, bank->W);
        if (valid && !pgsp::valid_ok(valid, bank->H, bank->W))
            return pg_fail(h, PG_EINVAL, "%s: valid (%d, %d, %d, %d) is inverted or outside the %d x %d frame", who, valid[0], valid[1], valid[2],
                           valid[3], bank->H, bank->W);
    }
    if (pg_misaligned(rgb, sizeof(float)) || pg_misaligned(sums, sizeof(double)))
        return pg_fail(h, PG_EINVAL, "%s: rgb / sums are not aligned to their element", who);
    const uint8_t* bg = nullptr;
    if (flags & PG_METRICS_BG) {
        if (!bank->bkgds || !bank->bkgd_idxs || bank->n_bkgd <= 0) return pg_fail(h, PG_EINVAL, "%s: PG_METRICS_BG on a bank without backgrounds", who);
        if (!bank->masks) return pg_fail(h, PG_EINVAL, "%s: PG_METRICS_BG on a bank without masks", who);
        const int32_t b = bank->bkgd_idxs[img_row];
        if (b < 0 || b >= bank->n_bkgd) return pg_fail(h, PG_EINVAL, "%s: bkgd_idxs[%d] = %d is outside [0, %lld)", who, img_row, b, (long long)bank->n_bkgd);
        bg = bank->bkgds + (size_t)b * bank->P * 3;
    }
    MetricsState* s = nullptr;
    PG_TRY(pg_state(h, s));
    const int w = box[2] - box[0], hh = box[3] - box[1];
    const int ntx = pgsp::tiles_along(w), nty = pgsp::tiles_along(hh);
    const bool up = wide && (rgb_h != bank->H || rgb_w != bank->W), val = wide && valid;
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(pg_grow(h, s->slots, pgsp::slot_bytes(w, hh, val ? pgsp::SUMS_VAL : pgsp::SUMS), "frame metrics tile sums"));
    pgs::Args a{rgb, bank->imgs + (size_t)img_row * bank->P * 3, bank->masks ? bank->masks + (size_t)img_row * bank->P : nullptr, bg,
                bank->W, box[0], box[1], w, hh, ntx, {}, s->slots.as<double>(), bank->H, up ? rgb_h : bank->H, up ? rgb_w : bank->W,
                val ? valid[0] - box[0] : 0, val ? valid[1] - box[1] : 0, val ? valid[2] - box[0] : 0, val ? valid[3] - box[1] : 0};
    for (int t = 0; t < pgsp::WIN; ++t) a.taps[t] = (double)pgsp::TAPS[t];
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ntiles = ntx * nty;
    if (up && val) launch_tiles<true, true>(a, ntiles, st);
    else if (up) launch_tiles<true, false>(a, ntiles, st);
    else if (val) launch_tiles<false, true>(a, ntiles, st);
    else launch_tiles<false, false>(a, ntiles, st);
    PG_LAUNCH_CHECK(h, "frame metrics kernel");
    const double* slots = s->slots.as<const double>();
    if (!wide) hipLaunchKernelGGL((pgs::frame_metrics_sum_kernel<pgsp::SUMS, pgsp::SUMS>), dim3(1), dim3(64), 0, st, slots, ntiles, sums);
    else if (val) hipLaunchKernelGGL((pgs::frame_metrics_sum_kernel<pgsp::SUMS_VAL, pgsp::SUMS_VAL>), dim3(1), dim3(64), 0, st, slots, ntiles, sums);
    else hipLaunchKernelGGL((pgs::frame_metrics_sum_kernel<pgsp::SUMS, pgsp::SUMS_VAL>), dim3(1), dim3(64), 0, st, slots, ntiles, sums);
    PG_LAUNCH_CHECK(h, "frame metrics sum kernel");
    return PG_OK;
}

}  // namespace

extern "C" int pg_frame_metrics(pg_handle* h, void* stream, const pg_image_bank* bank, int32_t img_row, const int32_t box[4], const float* rgb,
                                int flags, double* sums) {
    return frame_metrics(h, "pg_frame_metrics", false, stream, bank, img_row, box, rgb, 0, 0, nullptr, flags, sums);
}

extern "C" int pg_frame_metrics_val(pg_handle* h, void* stream, const pg_image_bank* bank, int32_t img_row, const int32_t box[4],
                                    const float* rgb, int32_t rgb_h, int32_t rgb_w, const int32_t valid[4], int flags, double* sums) {
    return frame_metrics(h, "pg_frame_metrics_val", true, stream, bank, img_row, box, rgb, rgb_h, rgb_w, valid, flags, sums);
}
