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

__global__ __launch_bounds__(THREADS) void frame_metrics_kernel(Args a) {
    __shared__ float sx[3 * PLANE], sy[3 * PLANE];       // frame and ground truth, [channel][row][col]
    __shared__ double hm[5 * HROWS];                     // the row pass of one channel, [moment][row][map col]
    __shared__ uint8_t sm[PLANE];                        // mask > 0
    __shared__ double red[WAVES][4];
    __shared__ int redi[WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx = blockIdx.x % a.ntx, ty = blockIdx.x / a.ntx;
    const Span xs = tile_span(a.w, tx), ys = tile_span(a.h, ty);

    // stage: a wave per row, a lane per (col, channel) -- the row's 3 sn consecutive floats / bytes of the frame and the image
    double se = 0.0, se_fg = 0.0, ssim = 0.0, ssim_fg = 0.0;
    int n_fg = 0, n_fg_map = 0;
    for (int r = wv; r < STAGE; r += WAVES) {
        const long long prow = (long long)(a.y0 + ys.s0 + r) * a.W + (a.x0 + xs.s0);
        for (int k = lane; k < STAGE * 3; k += 64) {
            const int col = k / 3, ch = k - col * 3;
            float xv = 0.0f, yv = 0.0f;
            bool m = false;
            if (r < ys.sn && col < xs.sn) {
                const long long p = prow + col;
                xv = a.rgb[p * 3 + ch];
                m = a.mask && a.mask[p] > 0;
                uint8_t b = a.img[p * 3 + ch];
                if (a.bg && !m) b = a.bg[p * 3 + ch];
                yv = __fdiv_rn((float)b, 255.0f);
                if (r < ys.own && col < xs.own) {
                    const double d = (double)yv - (double)xv;
                    se += d * d;
                    if (m) { se_fg += d * d; ++n_fg; }
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
                }
            }
            __syncthreads();
        }
    }

    // lanes by shuffles, then the waves in index order
    se = wave_sum(se); se_fg = wave_sum(se_fg); ssim = wave_sum(ssim); ssim_fg = wave_sum(ssim_fg);
    n_fg = wave_sum(n_fg); n_fg_map = wave_sum(n_fg_map);
    if (lane == 0) {
        red[wv][0] = se; red[wv][1] = se_fg; red[wv][2] = ssim; red[wv][3] = ssim_fg;
        redi[wv][0] = n_fg; redi[wv][1] = n_fg_map;
    }
    __syncthreads();
    if (tid == 0) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        int c[2] = {0, 0};
        for (int w = 0; w < WAVES; ++w) {
            for (int q = 0; q < 4; ++q) s[q] += red[w][q];
            c[0] += redi[w][0]; c[1] += redi[w][1];
        }
        double* o = a.slots + slot_offset(a.ntx, tx, ty);
        o[0] = 3.0 * xs.own * ys.own; o[1] = s[0]; o[2] = (double)c[0]; o[3] = s[1];     // (n_fg: a lane per channel has counted 3 m)
        o[4] = 3.0 * xs.map * ys.map; o[5] = s[2]; o[6] = (double)c[1]; o[7] = s[3];
    }
}

// sums[c] = slots[0][c] + slots[1][c] + ... in this order, a lane per sum
__global__ __launch_bounds__(64) void frame_metrics_sum_kernel(const double* __restrict__ slots, int ntiles, double* __restrict__ sums) {
    const int c = threadIdx.x;
    if (c >= SUMS) return;
    double acc = 0.0;
#pragma unroll 8
    for (int t = 0; t < ntiles; ++t) acc += slots[(size_t)t * SUMS + c];
    sums[c] = acc;
}

}  // namespace pgs

// ---- the host side: the entry point of the C ABI and what it keeps in the handle ------------------------------------------------------
namespace {

// the tiles' partial sums.  One buffer per handle: calls on one handle are serialised by the caller, and calls enqueued on different
// streams have to be ordered by the caller as well.
struct MetricsState {
    DevBuf slots;
};

}  // namespace

void pg_metrics_release(pg_handle* h) {
    if (!h || !h->metrics) return;
    auto* s = static_cast<MetricsState*>(h->metrics);
    pg_release(s->slots);
    delete s;
    h->metrics = nullptr;
}

extern "C" int pg_frame_metrics(pg_handle* h, void* stream, const pg_image_bank* bank, int32_t img_row, const int32_t box[4], const float* rgb,
                                int flags, double* sums) {
    const char* who = "pg_frame_metrics";
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
    if (reinterpret_cast<uintptr_t>(rgb) % sizeof(float) || reinterpret_cast<uintptr_t>(sums) % sizeof(double))
        return pg_fail(h, PG_EINVAL, "%s: rgb / sums are not aligned to their element", who);
    const uint8_t* bg = nullptr;
    if (flags & PG_METRICS_BG) {
        if (!bank->bkgds || !bank->bkgd_idxs || bank->n_bkgd <= 0) return pg_fail(h, PG_EINVAL, "%s: PG_METRICS_BG on a bank without backgrounds", who);
        if (!bank->masks) return pg_fail(h, PG_EINVAL, "%s: PG_METRICS_BG on a bank without masks", who);
        const int32_t b = bank->bkgd_idxs[img_row];
        if (b < 0 || b >= bank->n_bkgd) return pg_fail(h, PG_EINVAL, "%s: bkgd_idxs[%d] = %d is outside [0, %lld)", who, img_row, b, (long long)bank->n_bkgd);
        bg = bank->bkgds + (size_t)b * bank->P * 3;
    }
    if (!h->metrics) h->metrics = new MetricsState();
    auto* s = static_cast<MetricsState*>(h->metrics);
    const int w = box[2] - box[0], hh = box[3] - box[1];
    const int ntx = pgsp::tiles_along(w), nty = pgsp::tiles_along(hh);
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(pg_grow(h, s->slots, pgsp::slot_bytes(w, hh), "frame metrics tile sums"));
    pgs::Args a{rgb, bank->imgs + (size_t)img_row * bank->P * 3, bank->masks ? bank->masks + (size_t)img_row * bank->P : nullptr, bg,
                bank->W, box[0], box[1], w, hh, ntx, {}, s->slots.as<double>()};
    for (int t = 0; t < pgsp::WIN; ++t) a.taps[t] = (double)pgsp::TAPS[t];
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pgs::frame_metrics_kernel, dim3((unsigned)(ntx * nty)), dim3(pgs::THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "frame metrics kernel");
    hipLaunchKernelGGL(pgs::frame_metrics_sum_kernel, dim3(1), dim3(64), 0, st, s->slots.as<const double>(), ntx * nty, sums);
    PG_LAUNCH_CHECK(h, "frame metrics sum kernel");
    return PG_OK;
}
