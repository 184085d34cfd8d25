// pg_batch.hip -- training batches from an image bank that lives on the device:
//   pixel_count_kernel / pixel_scan_kernel / pixel_emit_kernel : the valid pixels of every image's sampling mask, indexed once -- counts
//                                           per tile of 4096 pixels from wave ballots, an ordered scan of an image's tiles, then every
//                                           valid pixel's id at its ballot prefix: np.where(mask > 0) of every image, back to back
//   sample_pixels_kernel                  : a uniformly random k-subset of an image's valid pixels in ascending order (Floyd's algorithm
//                                           at the caller's draws, one wave per image): np.sort(np.random.choice(valid, k, replace=False))
//   batch_gather_kernel                   : target colours, masks, backgrounds and rays of the chosen pixels, one thread per ray
// No atomics: every output slot comes from a scan or a rank, two runs give the same bytes.  Image addressing is 64-bit throughout (a bank
// is tens of GB).  Plain integer and fp32 vector code; the fp32 operations are the _rn intrinsics so that nothing is contracted.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cstring>

#include "pg_handle.h"
#include "pg_launch.h"

namespace pgb {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TILE = 4096;               // pixels per workgroup: wave w owns pixels [w, w + 1) * SEG of it, 64 at a time
constexpr int SEG = TILE / WAVES;
constexpr int ROUNDS = SEG / 64;
constexpr int MAX_K = 1024;

__device__ __forceinline__ int tile_total(const int* wsum) { return wsum[0] + wsum[1] + wsum[2] + wsum[3]; }
static_assert(WAVES == 4, "tile_total adds four waves");

// tile_cnt[f * ntiles + t] = valid pixels of image f in [t, t + 1) * TILE
__global__ __launch_bounds__(THREADS) void pixel_count_kernel(const uint8_t* __restrict__ masks, long long F, long long P, int ntiles,
                                                              int* __restrict__ tile_cnt) {
    __shared__ int wsum[WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long tiles = F * ntiles;
    for (long long T = blockIdx.x; T < tiles; T += gridDim.x) {
        const long long f = T / ntiles;
        const int t = (int)(T - f * ntiles);
        const uint8_t* row = masks + f * P;
        const long long p0 = (long long)t * TILE + w * SEG + lane;
        int c = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const long long p = p0 + r * 64;
            const bool v = p < P && row[p] > 0;
            c += __popcll(__ballot(v));
        }
        if (lane == 0) wsum[w] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[T] = tile_total(wsum);
        __syncthreads();
    }
}

// per image: its tiles' counts -> their exclusive prefix, in place; counts[f] = the image's total.  One workgroup walks an image's
// tiles in order, 256 at a time with a carry.
__global__ __launch_bounds__(THREADS) void pixel_scan_kernel(int* __restrict__ tile_cnt, long long F, int ntiles, long long* __restrict__ counts) {
    __shared__ int wsum[WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        int* tc = tile_cnt + f * ntiles;
        int carry = 0;
        for (int t0 = 0; t0 < ntiles; t0 += THREADS) {
            const int t = t0 + (int)threadIdx.x;
            const int v = t < ntiles ? tc[t] : 0;
            int inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            if (lane == 63) wsum[w] = inc;
            __syncthreads();
            int before = 0;
            for (int i = 0; i < w; ++i) before += wsum[i];
            if (t < ntiles) tc[t] = carry + before + inc - v;
            carry += tile_total(wsum);
            __syncthreads();
        }
        if (threadIdx.x == 0) counts[f] = carry;
    }
}

// ids[start[f] + (rank of pixel p among image f's valid pixels)] = p.  The slot is the image's start + the tile's offset + the waves
// before this one + the rounds before this one + the ballot's bits below the lane.  A mask that changed since the count cannot move a
// store outside the image's range: slots at or past start[f + 1] are dropped.
__global__ __launch_bounds__(THREADS) void pixel_emit_kernel(const uint8_t* __restrict__ masks, long long F, long long P, int ntiles,
                                                             const int* __restrict__ tile_off, const long long* __restrict__ start,
                                                             int* __restrict__ ids) {
    __shared__ int wsum[WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long tiles = F * ntiles;
    for (long long T = blockIdx.x; T < tiles; T += gridDim.x) {
        const long long f = T / ntiles;
        const int t = (int)(T - f * ntiles);
        const uint8_t* row = masks + f * P;
        const long long p0 = (long long)t * TILE + w * SEG + lane;
        unsigned long long b[ROUNDS];
        int c = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const long long p = p0 + r * 64;
            const bool v = p < P && row[p] > 0;
            b[r] = __ballot(v);
            c += __popcll(b[r]);
        }
        if (lane == 0) wsum[w] = c;
        __syncthreads();
        int before = 0;
        for (int i = 0; i < w; ++i) before += wsum[i];
        const long long end = start[f + 1];
        long long off = start[f] + tile_off[T] + before;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if ((b[r] >> lane) & 1ull) {
                const long long slot = off + __popcll(b[r] & below);
                if (slot < end) ids[slot] = (int)(p0 + r * 64);
            }
            off += __popcll(b[r]);
        }
        __syncthreads();
    }
}

// One wave per batch image a (image img_rows[a], m valid pixels, draws u = draws[a, :]).  Floyd's algorithm in the order of the draws:
// for j = m - k .. m - 1, t = min(floor(u (j + 1)), j); t if it is not chosen yet, else j.  The chosen ranks sit in LDS; membership is
// a wave-strided compare and a ballot; the sort is rank by counting (the ranks are distinct).
__global__ __launch_bounds__(64) void sample_pixels_kernel(const int* __restrict__ ids, const long long* __restrict__ start,
                                                           const int* __restrict__ img_rows, int k, const double* __restrict__ draws,
                                                           int* __restrict__ pix) {
    __shared__ int chosen[MAX_K];
    const long long a = blockIdx.x;
    const int lane = threadIdx.x;
    const int img = img_rows[a];
    const long long s0 = start[img];
    const long long m = start[img + 1] - s0;
    if (m < k) return;                                   // (refused on the host from its counts; never an index outside the image)
    const double* u = draws + a * k;
    for (int i = 0; i < k; ++i) {
        const long long j = m - k + i;
        long long t = (long long)floor(u[i] * (double)(j + 1));
        if (!(t >= 0)) t = 0;
        if (t > j) t = j;
        bool hit = false;
        for (int x = lane; x < i; x += 64) hit |= chosen[x] == (int)t;
        const bool found = __ballot(hit) != 0ull;
        if (lane == 0) chosen[i] = (int)(found ? j : t);
        __syncthreads();
    }
    for (int x = lane; x < k; x += 64) {
        const int e = chosen[x];
        int rank = 0;
        for (int y = 0; y < k; ++y) rank += chosen[y] < e ? 1 : 0;
        pix[a * k + rank] = ids[s0 + e];
    }
}

__device__ __forceinline__ float u8_unit(uint8_t v) { return __fdiv_rn((float)v, 255.0f); }

// ray r = a k + b: pixel pix[r] of image rows[a], camera rows[n_img + a], background rows[2 n_img + a].  A pixel id outside [0, P)
// reads nothing and writes NaN.
__global__ __launch_bounds__(THREADS) void batch_gather_kernel(pgk::BatchGather g) {
    const long long n = g.n_img * g.k;
    const long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const long long a = r / g.k;
    const long long img = g.rows[a], cam = g.rows[g.n_img + a];
    const long long p = g.pix[r];
    const bool ok = p >= 0 && p < g.P;
    const float nan = __int_as_float(0x7fc00000);

    float fg = nan, rgb[3] = {nan, nan, nan}, bg[3] = {nan, nan, nan};
    if (ok) {
        const uint8_t* px = g.imgs + (img * g.P + p) * 3;
        fg = (float)g.masks[img * g.P + p];
        for (int c = 0; c < 3; ++c) rgb[c] = u8_unit(px[c]);
        if (g.bkgds) {
            const long long bk = g.rows[2 * g.n_img + a];
            const uint8_t* bx = g.bkgds + (bk * g.P + p) * 3;
            for (int c = 0; c < 3; ++c) bg[c] = u8_unit(bx[c]);
            if (g.mask_img) {
                const float inv = __fsub_rn(1.0f, fg);
                for (int c = 0; c < 3; ++c) rgb[c] = __fadd_rn(__fmul_rn(rgb[c], fg), __fmul_rn(inv, bg[c]));
            }
        }
    }
    g.fgs[r] = fg;
    for (int c = 0; c < 3; ++c) g.target[r * 3 + c] = rgb[c];
    if (g.bgs) for (int c = 0; c < 3; ++c) g.bgs[r * 3 + c] = bg[c];

    const float* M = g.c2ws + cam * 12;                  // [3,4] row-major
    const float fx = g.focals[cam * 2], fy = g.focals[cam * 2 + 1];
    float o[3] = {M[3], M[7], M[11]}, d[3] = {nan, nan, nan};
    if (ok) {
        const int pi = (int)p;                           // P < 2^31
        const float row = (float)(pi / g.W), col = (float)(pi % g.W);
        float x, y;
        if (g.centers) {
            x = __fdiv_rn(__fsub_rn(col, g.centers[cam * 2]), fx);
            y = __fdiv_rn(__fadd_rn(-row, g.centers[cam * 2 + 1]), fy);
        } else {
            x = __fdiv_rn(__fsub_rn(col, __fmul_rn((float)g.W, 0.5f)), fx);
            y = __fdiv_rn(-__fsub_rn(row, __fmul_rn((float)g.H, 0.5f)), fy);
        }
        for (int c = 0; c < 3; ++c)
            d[c] = __fadd_rn(__fadd_rn(__fmul_rn(x, M[c * 4]), __fmul_rn(y, M[c * 4 + 1])), __fmul_rn(-1.0f, M[c * 4 + 2]));
    }
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
    float* q = g.ray_batch + r * 11;
    for (int c = 0; c < 3; ++c) {
        g.rays_o[r * 3 + c] = o[c];
        g.rays_d[r * 3 + c] = d[c];
        q[c] = o[c];
        q[3 + c] = d[c];
        q[8 + c] = __fdiv_rn(d[c], nrm);
    }
    q[6] = 0.0f;
    q[7] = 1.0f;
}

inline unsigned grid_for(long long items) {
    const long long cap = 1ll << 20;
    return (unsigned)(items < 1 ? 1 : items < cap ? items : cap);
}

}  // namespace pgb

extern "C" {

int pg_batch_tile_pixels(void) { return pgb::TILE; }
int pg_batch_max_pixels(void) { return pgb::MAX_K; }

int pg_launch_pixel_count(const uint8_t* masks, long long F, long long P, int* tile_cnt, long long* counts, void* stream) {
    using namespace pgb;
    const int ntiles = (int)((P + TILE - 1) / TILE);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pixel_count_kernel, dim3(grid_for(F * ntiles)), dim3(THREADS), 0, st, masks, F, P, ntiles, tile_cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pixel_scan_kernel, dim3(grid_for(F)), dim3(THREADS), 0, st, tile_cnt, F, ntiles, counts);
    return (int)hipGetLastError();
}

int pg_launch_pixel_emit(const uint8_t* masks, long long F, long long P, const int* tile_off, const long long* start, int* ids, void* stream) {
    using namespace pgb;
    const int ntiles = (int)((P + TILE - 1) / TILE);
    hipLaunchKernelGGL(pixel_emit_kernel, dim3(grid_for(F * ntiles)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), masks, F, P, ntiles,
                       tile_off, start, ids);
    return (int)hipGetLastError();
}

int pg_launch_sample_pixels(const int* ids, const long long* start, const int* img_rows, long long n_img, int k, const double* draws, int* pix,
                            void* stream) {
    hipLaunchKernelGGL(pgb::sample_pixels_kernel, dim3((unsigned)n_img), dim3(64), 0, static_cast<hipStream_t>(stream), ids, start, img_rows, k,
                       draws, pix);
    return (int)hipGetLastError();
}

int pg_launch_batch_gather(const pgk::BatchGather* g, void* stream) {
    const long long n = g->n_img * g->k;
    hipLaunchKernelGGL(pgb::batch_gather_kernel, dim3((unsigned)((n + pgb::THREADS - 1) / pgb::THREADS)), dim3(pgb::THREADS), 0,
                       static_cast<hipStream_t>(stream), *g);
    return (int)hipGetLastError();
}

}  // extern "C"

// ---- the host side: the four entry points of the C ABI and what they keep in the handle ---------------------------------------------
namespace {

// what the four entry points keep in the handle: the tile offsets of the last pg_pixel_index_count (and what they were counted on),
// and the upload ring (pg_handle.h) of a call's image rows
struct BatchState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_BATCH;
    ~BatchState() override { pg_release(tiles); pg_ring_release(rows); }
    DevBuf tiles;
    const void* masks = nullptr;
    int64_t F = 0, P = 0;
    UploadRing rows;
};

// `words` (checked by the caller) -> the next slot's device buffer, on stream st
int batch_upload(pg_handle* h, const std::vector<int32_t>& words, hipStream_t st, const int** dev) {
    const void* p = nullptr;
    BatchState* s = nullptr;
    PG_TRY(pg_state(h, s));
    PG_TRY(pg_ring_upload(h, s->rows, words.data(), words.size() * sizeof(int32_t),
                          (words.size() + words.size() / 2 + 64) * sizeof(int32_t), "batch row buffer", st, &p));
    *dev = static_cast<const int*>(p);
    return PG_OK;
}

int check_index_args(pg_handle* h, const char* who, const void* masks, int64_t F, int64_t P) {
    if (!masks) return pg_fail(h, PG_EINVAL, "%s: sampling_masks is null", who);
    if (F <= 0 || P <= 0) return pg_fail(h, PG_EINVAL, "%s: F (%lld) and P (%lld) must be positive", who, (long long)F, (long long)P);
    if (P > 0x7ffffffell) return pg_fail(h, PG_EINVAL, "%s: at most 2^31 - 2 pixels per image (the ids are int32)", who);
    const int64_t ntiles = (P + pg_batch_tile_pixels() - 1) / pg_batch_tile_pixels();
    if (F > (int64_t)(0x7fffffffffffll / ntiles)) return pg_fail(h, PG_EINVAL, "%s: F * P is too large", who);
    return PG_OK;
}

int check_rows(pg_handle* h, const char* who, const char* what, const int32_t* rows, int64_t n, int64_t bound) {
    for (int64_t a = 0; a < n; ++a)
        if (rows[a] < 0 || rows[a] >= bound)
            return pg_fail(h, PG_EINVAL, "%s: %s[%lld] = %d is outside [0, %lld)", who, what, (long long)a, rows[a], (long long)bound);
    return PG_OK;
}

}  // namespace

extern "C" {

int pg_pixel_index_count(pg_handle* h, void* stream, const uint8_t* sampling_masks, int64_t F, int64_t P, int64_t* counts) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    PG_TRY(check_index_args(h, "pg_pixel_index_count", sampling_masks, F, P));
    if (!counts) return pg_fail(h, PG_EINVAL, "pg_pixel_index_count: counts is null");
    BatchState* s = nullptr;
    PG_TRY(pg_state(h, s));
    s->masks = nullptr;
    const int64_t ntiles = (P + pg_batch_tile_pixels() - 1) / pg_batch_tile_pixels();
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(pg_grow(h, s->tiles, (size_t)(F * ntiles) * sizeof(int), "pixel index tile counts"));
    PG_TRY_LAUNCH(h, "pixel count kernels",
                  pg_launch_pixel_count(sampling_masks, F, P, s->tiles.as<int>(), reinterpret_cast<long long*>(counts), stream));
    s->masks = sampling_masks; s->F = F; s->P = P;
    return PG_OK;
}

int pg_pixel_index_emit(pg_handle* h, void* stream, const uint8_t* sampling_masks, int64_t F, int64_t P, const int64_t* start,
                        int64_t total, int32_t* ids) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    PG_TRY(check_index_args(h, "pg_pixel_index_emit", sampling_masks, F, P));
    if (!start || total < 0 || (total > 0 && !ids)) return pg_fail(h, PG_EINVAL, "pg_pixel_index_emit: null start / ids or negative total");
    BatchState* s = nullptr;
    PG_TRY(pg_state(h, s));
    if (s->masks != sampling_masks || s->F != F || s->P != P)
        return pg_fail(h, PG_ESTATE, "pg_pixel_index_emit: masks, F and P are not those of the last pg_pixel_index_count");
    if (total == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY_LAUNCH(h, "pixel emit kernel", pg_launch_pixel_emit(sampling_masks, F, P, s->tiles.as<const int>(),
                                                               reinterpret_cast<const long long*>(start), ids, stream));
    return PG_OK;
}

int pg_batch_sample_pixels(pg_handle* h, void* stream, const int32_t* ids, const int64_t* start, const int64_t* counts, int64_t F,
                           const int32_t* img_rows, int64_t n_img, int k, const double* draws, int32_t* pixel_idxs) {
    const char* who = "pg_batch_sample_pixels";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!ids || !start || !counts || !img_rows || !draws || !pixel_idxs) return pg_fail(h, PG_EINVAL, "%s: null argument", who);
    if (F <= 0) return pg_fail(h, PG_EINVAL, "%s: F (%lld) must be positive", who, (long long)F);
    if (k < 1 || k > pg_batch_max_pixels()) return pg_fail(h, PG_EINVAL, "%s: k = %d is outside [1, %d]", who, k, pg_batch_max_pixels());
    if (n_img < 0 || n_img > 0x7ffffffell / k) return pg_fail(h, PG_EINVAL, "%s: n_img (%lld) negative or n_img * k above 2^31 - 2", who, (long long)n_img);
    PG_TRY(check_rows(h, who, "img_rows", img_rows, n_img, F));
    for (int64_t a = 0; a < n_img; ++a)
        if (k > counts[img_rows[a]])
            return pg_fail(h, PG_EINVAL, "%s: image %d has %lld valid pixels, fewer than k = %d", who, img_rows[a], (long long)counts[img_rows[a]], k);
    if (n_img == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int* d_rows = nullptr;
    PG_TRY(batch_upload(h, std::vector<int32_t>(img_rows, img_rows + n_img), st, &d_rows));
    PG_TRY_LAUNCH(h, "pixel sampler kernel",
                  pg_launch_sample_pixels(ids, reinterpret_cast<const long long*>(start), d_rows, n_img, k, draws, pixel_idxs, stream));
    return PG_OK;
}

int pg_batch_gather(pg_handle* h, void* stream, const pg_image_bank* bank, const int32_t* img_rows, const int32_t* cam_rows, int64_t n_img,
                    int k, const int32_t* pixel_idxs, float* target_s, float* fgs, float* bgs, float* rays_o, float* rays_d, float* ray_batch) {
    const char* who = "pg_batch_gather";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!bank || !img_rows || !pixel_idxs || !target_s || !fgs || !rays_o || !rays_d || !ray_batch) return pg_fail(h, PG_EINVAL, "%s: null argument", who);
    if (!bank->imgs || !bank->masks || !bank->c2ws || !bank->focals) return pg_fail(h, PG_EINVAL, "%s: the bank's imgs / masks / c2ws / focals are required", who);
    if (bank->F <= 0 || bank->P <= 0 || bank->n_cam <= 0) return pg_fail(h, PG_EINVAL, "%s: F, P and n_cam must be positive", who);
    if (bank->H <= 0 || bank->W <= 0 || (int64_t)bank->H * bank->W != bank->P || bank->P > 0x7ffffffell)
        return pg_fail(h, PG_EINVAL, "%s: H x W = %d x %d is not P = %lld", who, bank->H, bank->W, (long long)bank->P);
    if (bank->bkgds && (!bank->bkgd_idxs || bank->n_bkgd <= 0)) return pg_fail(h, PG_EINVAL, "%s: backgrounds without bkgd_idxs / n_bkgd", who);
    if (bgs && !bank->bkgds) return pg_fail(h, PG_EINVAL, "%s: bgs asked for from a bank without backgrounds", who);
    if (k < 1 || k > pg_batch_max_pixels()) return pg_fail(h, PG_EINVAL, "%s: k = %d is outside [1, %d]", who, k, pg_batch_max_pixels());
    if (n_img < 0 || n_img > 0x7ffffffell / k) return pg_fail(h, PG_EINVAL, "%s: n_img (%lld) negative or n_img * k above 2^31 - 2", who, (long long)n_img);
    PG_TRY(check_rows(h, who, "img_rows", img_rows, n_img, bank->F));
    PG_TRY(check_rows(h, who, "cam_rows", cam_rows ? cam_rows : img_rows, n_img, bank->n_cam));
    std::vector<int32_t> rows((size_t)n_img * 3, 0);
    for (int64_t a = 0; a < n_img; ++a) {
        rows[a] = img_rows[a];
        rows[n_img + a] = (cam_rows ? cam_rows : img_rows)[a];
        if (bank->bkgds) {
            const int32_t b = bank->bkgd_idxs[img_rows[a]];
            if (b < 0 || b >= bank->n_bkgd)
                return pg_fail(h, PG_EINVAL, "%s: bkgd_idxs[%d] = %d is outside [0, %lld)", who, img_rows[a], b, (long long)bank->n_bkgd);
            rows[2 * n_img + a] = b;
        }
    }
    if (n_img == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int* d_rows = nullptr;
    PG_TRY(batch_upload(h, rows, st, &d_rows));
    pgk::BatchGather g{bank->imgs, bank->masks, bank->bkgds, bank->c2ws, bank->focals, bank->centers, bank->P, bank->H, bank->W,
                       bank->bkgds ? bank->mask_img : 0, d_rows, n_img, k, pixel_idxs, target_s, fgs, bgs, rays_o, rays_d, ray_batch};
    PG_TRY_LAUNCH(h, "batch gather kernel", pg_launch_batch_gather(&g, stream));
    return PG_OK;
}

}  // extern "C"
