// pg_regressor.hip -- the regressor's input batch from uint8 pictures on the device: per item crop, divide by 255,
// normalise, and skimage.transform.resize(image, (3, R, R), anti_aliasing=True) -- a mirrored Gaussian of sigma = (n / R - 1) / 2
// per axis, then order-1 interpolation at pixel centres with mirrored borders (run_gan.py:1636-1735, 2057-2081).
//   regressor_input_kernel : a workgroup takes a TY x TX tile of one item's output, all three channels.  Per axis the Gaussian and the
//                            interpolation are ONE filter of 2 r + 2 taps per output sample (weights formed in double, rounded to
//                            float32 once).  The horizontal filter reads the uint8 pixels (coalesced along x, mirrored at the read,
//                            normalised by one fma) and leaves [source rows of a band] x [TX x 3] floats in LDS; the vertical
//                            filter runs from LDS and stores 32 consecutive floats per (channel, row).  The tile's output rows are
//                            taken in bands whose source rows fit the LDS rows, so a 16-fold downscale (62 taps) and an upscale
//                            (2 taps) share a launch; every band holds at least one output row.
// No atomics; an output sample is one thread's two fma chains in a fixed order, so an item's bytes depend on nothing but the item.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pg_handle.h"

namespace pgr {

constexpr int THREADS = 256;
constexpr int TX = 32, TY = 16;                  // the output tile
constexpr int ROW = TX * 3;                      // floats of an LDS row: (column, channel), channel fastest
constexpr int MAX_RES = 512, MAX_SCALE = 16;     // 1 <= R <= 512, a crop side n <= 16 R
constexpr int MAX_RADIUS = 30;                   // int(4 (16 - 1) / 2 + 0.5)
constexpr int MAX_TAPS = 2 * MAX_RADIUS + 2;
constexpr int LDS_ROWS = 64;                     // source rows of a band
static_assert(LDS_ROWS >= MAX_TAPS, "a band holds at least one output row's taps");
static_assert(3 * (MAX_RES * MAX_SCALE - 1) <= 0xffff, "the column offsets are 16-bit");
static_assert((2 * MAX_RADIUS + 1) * 2 * sizeof(double) <= LDS_ROWS * ROW * sizeof(float), "the Gaussians borrow the band's rows");

struct Args {
    const uint8_t* pixels;
    const pg_crop_item* items;
    float* out;
    int R, tiles_x, tiles_y;
    float scale[3], shift[3];                    // v = fma(u8, scale, shift) = (u8 / 255 - mean) / std
};

// reflection about the centres of the first and the last of n pixels (scipy.ndimage 'mirror')
__device__ __forceinline__ int mirror(int i, int n) {
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int j = i % p;
    if (j < 0) j += p;
    return j < n ? j : p - j;
}

__device__ __forceinline__ int radius_of(int n, int R, double* sigma) {
    const double s = (double)n / (double)R;
    *sigma = fmax(0.0, (s - 1.0) / 2.0);
    return (int)(4.0 * *sigma + 0.5);
}

// tap j (0 .. 2 r + 1) of output sample o of an axis n -> R reads source index first + j with weight
// (1 - t) k[j] + t k[j - 1], k the normalised Gaussian over -r .. r stored from index 0 (gauss: its unnormalised values, r > 0)
__device__ __forceinline__ double sample_position(int o, int n, int R, int* i0) {
    const double x = ((double)o + 0.5) * (double)n / (double)R - 0.5;
    const double f = floor(x);
    *i0 = (int)f;
    return x - f;
}

__device__ __forceinline__ float tap_weight(int j, int r, double t, const double* gauss, double sum) {
    if (r == 0) return (float)(j == 0 ? 1.0 - t : t);
    const double a = j <= 2 * r ? gauss[j] / sum : 0.0;
    const double b = j >= 1 ? gauss[j - 1] / sum : 0.0;
    return (float)((1.0 - t) * a + t * b);
}

__global__ __launch_bounds__(THREADS) void regressor_input_kernel(Args a) {
    __shared__ float band[LDS_ROWS * ROW];       // [source row of the band][column, channel] after the horizontal filter
    __shared__ float wx[MAX_TAPS * TX];          // [tap][column]
    __shared__ uint16_t ox3[MAX_TAPS * TX];      // [tap][column]: 3 x the mirrored source column of the crop
    __shared__ float wy[MAX_TAPS * TY];          // [tap][row]
    __shared__ int first_y[TY];                  // the (unmirrored) source row of an output row's tap 0

    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int item = blockIdx.x / tiles;
    const int tile = blockIdx.x - item * tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int R = a.R;
    const int o_x0 = tx * TX, o_y0 = ty * TY;
    const int cnt_x = min(TX, R - o_x0), cnt_y = min(TY, R - o_y0);

    const pg_crop_item it = a.items[item];
    const int w = it.x1 - it.x0, h = it.y1 - it.y0;
    double sig_x, sig_y;
    const int r_x = radius_of(w, R, &sig_x), r_y = radius_of(h, R, &sig_y);
    const int taps_x = 2 * r_x + 2, taps_y = 2 * r_y + 2;

    // ---- the two axes' filters, in double ----
    double* gauss_x = reinterpret_cast<double*>(band);
    double* gauss_y = gauss_x + 2 * MAX_RADIUS + 1;
    if (r_x > 0 && tid <= 2 * r_x) { const double d = (double)(tid - r_x); gauss_x[tid] = exp(-(d * d) / (2.0 * sig_x * sig_x)); }
    if (r_y > 0 && tid <= 2 * r_y) { const double d = (double)(tid - r_y); gauss_y[tid] = exp(-(d * d) / (2.0 * sig_y * sig_y)); }
    __syncthreads();
    double sum_x = 1.0, sum_y = 1.0;
    if (r_x > 0 && tid < taps_x * TX) { sum_x = 0.0; for (int j = 0; j <= 2 * r_x; ++j) sum_x += gauss_x[j]; }
    if (r_y > 0 && tid < taps_y * TY) { sum_y = 0.0; for (int j = 0; j <= 2 * r_y; ++j) sum_y += gauss_y[j]; }
    for (int idx = tid; idx < taps_x * TX; idx += THREADS) {
        const int j = idx / TX, l = idx - j * TX;
        float wt = 0.0f;
        int col = 0;
        if (l < cnt_x) {
            int i0;
            const double t = sample_position(o_x0 + l, w, R, &i0);
            wt = tap_weight(j, r_x, t, gauss_x, sum_x);
            col = mirror(i0 - r_x + j, w);
        }
        wx[idx] = wt;
        ox3[idx] = (uint16_t)(3 * col);
    }
    for (int idx = tid; idx < taps_y * TY; idx += THREADS) {
        const int j = idx / TY, l = idx - j * TY;
        float wt = 0.0f;
        if (l < cnt_y) {
            int i0;
            const double t = sample_position(o_y0 + l, h, R, &i0);
            wt = tap_weight(j, r_y, t, gauss_y, sum_y);
            if (j == 0) first_y[l] = i0 - r_y;
        }
        wy[idx] = wt;
    }
    __syncthreads();                             // (also: the Gaussians are read, the band's rows are free)

    const uint8_t* img = a.pixels + it.offset;
    const long long W3 = (long long)it.W * 3;
    float* out = a.out + (long long)item * 3 * R * R;

    // ---- bands of output rows whose source rows fit the LDS rows ----
    int oa = 0;
    while (oa < cnt_y) {
        const int lo = first_y[oa];
        int ob = oa + 1;
        while (ob < cnt_y && first_y[ob] + taps_y - lo <= LDS_ROWS) ++ob;
        const int rows = first_y[ob - 1] + taps_y - lo;

        for (int idx = tid; idx < rows * ROW; idx += THREADS) {
            const int q = idx / ROW, e = idx - q * ROW;
            const int l = e / 3, c = e - l * 3;
            if (l >= cnt_x) continue;
            const uint8_t* src = img + (long long)(it.y0 + mirror(lo + q, h)) * W3 + (long long)it.x0 * 3 + c;
            const float sc = c == 0 ? a.scale[0] : c == 1 ? a.scale[1] : a.scale[2];      // (selects: no indexed copy of the arguments)
            const float sh = c == 0 ? a.shift[0] : c == 1 ? a.shift[1] : a.shift[2];
            float acc = 0.0f;
            for (int j = 0; j < taps_x; ++j)
                acc = fmaf(wx[j * TX + l], fmaf((float)src[ox3[j * TX + l]], sc, sh), acc);
            band[idx] = acc;
        }
        __syncthreads();

        for (int idx = tid; idx < (ob - oa) * 3 * TX; idx += THREADS) {
            const int l = idx % TX, k = idx / TX;
            const int c = k % 3, row = oa + k / 3;
            if (l >= cnt_x) continue;
            const float* col = band + (first_y[row] - lo) * ROW + l * 3 + c;
            float acc = 0.0f;
            for (int j = 0; j < taps_y; ++j) acc = fmaf(wy[j * TY + row], col[j * ROW], acc);
            out[((long long)c * R + o_y0 + row) * R + o_x0 + l] = acc;
        }
        __syncthreads();
        oa = ob;
    }
}

}  // namespace pgr

// ---- the host side ------------------------------------------------------------------------------------------------------------------
namespace {

// what pg_regressor_input keeps in the handle: the upload ring (pg_handle.h) of a call's crop items
struct RegressorState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_REGRESSOR;
    ~RegressorState() override { pg_ring_release(ring); }
    UploadRing ring;
};

}  // namespace

extern "C" int pg_regressor_input(pg_handle* h, void* stream, const uint8_t* pixels, int64_t n_bytes, const pg_crop_item* items, int32_t n,
                                  int32_t out_res, const float mean[3], const float stdev[3], float* out) {
    using namespace pgr;
    const char* who = "pg_regressor_input";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!pixels || !items || !mean || !stdev || !out) return pg_fail(h, PG_EINVAL, "%s: null argument", who);
    if (n_bytes <= 0 || n < 0) return pg_fail(h, PG_EINVAL, "%s: n_bytes (%lld) must be positive and n (%d) not negative", who, (long long)n_bytes, n);
    if (out_res < 1 || out_res > MAX_RES) return pg_fail(h, PG_EINVAL, "%s: out_res = %d is outside [1, %d]", who, out_res, MAX_RES);
    Args a{pixels, nullptr, out, out_res, (out_res + TX - 1) / TX, (out_res + TY - 1) / TY, {}, {}};
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(stdev[c]) || stdev[c] == 0.0f)
            return pg_fail(h, PG_EINVAL, "%s: mean[%d] = %g, std[%d] = %g: finite values and a std other than 0 expected", who, c, mean[c], c, stdev[c]);
        a.scale[c] = (float)(1.0 / (255.0 * (double)stdev[c]));
        a.shift[c] = (float)(-(double)mean[c] / (double)stdev[c]);
    }
    const int64_t tiles = (int64_t)a.tiles_x * a.tiles_y;
    if (n > 0x7fffffffll / tiles) return pg_fail(h, PG_EINVAL, "%s: n = %d items of %lld tiles are more than 2^31 - 1 workgroups", who, n, (long long)tiles);
    const int side = MAX_SCALE * out_res;
    for (int32_t i = 0; i < n; ++i) {
        const pg_crop_item& it = items[i];
        if (it.H < 1 || it.W < 1 || it.offset < 0 || it.offset >= n_bytes || (n_bytes - it.offset) / 3 / it.W < it.H)
            return pg_fail(h, PG_EINVAL, "%s: item %d: an image of %d x %d pixels at byte %lld leaves the %lld bytes of pixels", who, i, it.H, it.W,
                           (long long)it.offset, (long long)n_bytes);
        if (it.x0 < 0 || it.y0 < 0 || it.x0 >= it.x1 || it.y0 >= it.y1 || it.x1 > it.W || it.y1 > it.H)
            return pg_fail(h, PG_EINVAL, "%s: item %d: the box (%d, %d, %d, %d) is empty or leaves its %d x %d image", who, i, it.x0, it.y0, it.x1,
                           it.y1, it.H, it.W);
        if (it.x1 - it.x0 > side || it.y1 - it.y0 > side)
            return pg_fail(h, PG_EINVAL, "%s: item %d: a crop of %d x %d is more than %d times out_res = %d", who, i, it.y1 - it.y0, it.x1 - it.x0,
                           MAX_SCALE, out_res);
    }
    if (n == 0) return PG_OK;
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    RegressorState* s = nullptr;                                 // the items go up through the handle's ring: no wait for the stream
    PG_TRY(pg_state(h, s));
    const void* d_items = nullptr;
    PG_TRY(pg_ring_upload(h, s->ring, items, (size_t)n * sizeof(pg_crop_item),
                          ((size_t)n + (size_t)n / 2 + 16) * sizeof(pg_crop_item), "crop item buffer", st, &d_items));
    a.items = static_cast<const pg_crop_item*>(d_items);
    hipLaunchKernelGGL(regressor_input_kernel, dim3((unsigned)(n * tiles)), dim3(THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "regressor input kernel");
    return PG_OK;
}
