// pg_disc.hip -- the adversarial game of the PoseGen loop on the device (include/posegen_gan.h): the part-path pose
// discriminators (Disc_Joint_Path / Pos3dDiscriminator / Pos2dDiscriminator, run_gan.py:982-1046) forward and backward, the
// least-squares loss with get_discriminator_accuracy's count (:1101-1177) and Sample_from_Pool (:578-599).
//   disc_fwd_kernel    : one layer of every path in one launch.  A workgroup owns a 64 x 64 tile of (rows, output columns) of the path
//                        blockIdx.z; K goes through LDS in chunks of 16, round four accumulators; wave w owns rows 16 w .. 16 w + 15 of the tile and all four
//                        column tiles on v_mfma_f32_16x16x4_f32.  Both operands are K-contiguous (nn.Linear keeps W as [out,in]).
//                        Layer 1 gathers its rows from x through `sel`; bias and LeakyReLU in the epilogue; edge tiles predicated.
//   disc_head_kernel   : the mid -> 1 head, one wave per (row, path): lane l adds columns l, l + 64, ..., then a butterfly.
//   disc_bwd_data_kernel   : dH_prev = dZ W with the mask of the previous layer's tape in the epilogue (same tile, reduction over N).
//   disc_bwd_weight_kernel : dW = dZ^T H_prev (reduction over the rows, folded every ROW_CHUNK rows) and db = colsum(dZ), the latter in
//                        double from the dZ tile in LDS, by the first wave of the workgroups of column tile 0, rounded once.
//   disc_dx_kernel     : d_x from the paths' layer-1 input gradients, one thread per element, paths in order.
//   disc_loss_kernel, pool_exchange_kernel : see the header.
// A row of the batch meets only its own values: a reduction over K or N runs in an order that the row's position and B do not enter,
// so a row's bytes are the same alone, in a batch and in a permuted batch.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/posegen_gan.h"
#include "pg_handle.h"

namespace pgdc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int TILE = 64;                    // rows and columns of a workgroup's tile
constexpr int BK = 16;                      // the reduction's chunk through LDS
constexpr int LDT = BK + 1;                 // LDS row stride (odd: the 64 rows of a column land in different banks)
constexpr int ROW_CHUNK = 64;               // rows per partial of the weight gradients
constexpr int MAXP = PG_DISC_MAX_PATHS, MAXS = PG_DISC_MAX_POINTS;
constexpr int POOL_MAX_ITEMS = 8192;        // items of one pg_pool_exchange call (their effective slots sit in LDS: 4 bytes each)

// layer 1's operand: row b, column k of path p is x[b, sel[p][k / point_dim], k % point_dim]
struct Gather {
    const float* x;
    int n_points, point_dim;
    int8_t sel[MAXP][MAXS];
};

__device__ __forceinline__ float gathered(const Gather& g, int path, long long b, int k) {
    const int i = k / g.point_dim, c = k - i * g.point_dim;
    return g.x[((size_t)b * g.n_points + g.sel[path][i]) * g.point_dim + c];
}

// a [64, 16] tile whose 16 run along memory: thread t takes row t / 4, four values from column 4 (t % 4)
__device__ __forceinline__ void load_r_contig(float* s, const float* src, size_t ld, long long row0, long long rows, int r0, int R, int tid) {
    const int row = tid >> 2, rq = (tid & 3) * 4;
    const long long g = row0 + row;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (g < rows) {
        const float* p = src + (size_t)g * ld + r0 + rq;
        if (r0 + rq + 3 < R && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (r0 + rq + c < R) v[c] = p[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s[row * LDT + rq + c] = v[c];
}

// a [64, 16] tile whose 64 run along memory (element (j, r) at src[r * ld + j]): thread t takes j = t % 64 and r = t / 64 + 4 c
__device__ __forceinline__ void load_j_contig(float* s, const float* src, size_t ld, int j0, int J, long long r0, long long R, int tid) {
    const int j = tid & 63, rq = tid >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int r = rq + 4 * c;
        s[j * LDT + r] = (j0 + j < J && r0 + r < R) ? src[(size_t)(r0 + r) * ld + j0 + j] : 0.f;
    }
}

// the 16-deep chunk in LDS into the wave's four accumulators (rows 16 w + ., columns 16 t + .)
__device__ __forceinline__ void mma_chunk(const float* sa, const float* sb, int w, int l15, int l4, f32x4 (&acc)[4]) {
#pragma unroll
    for (int s = 0; s < BK / 4; ++s) {
        const float a = sa[(16 * w + l15) * LDT + 4 * s + l4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sb[(16 * t + l15) * LDT + 4 * s + l4], acc[t], 0, 0, 0);
    }
}

// A reduction over K (or N) goes round NACC accumulators, chunk c into accumulator c % NACC, and the four are added as a tree at the
// end: a float32 chain a quarter as long, which is what a blocked sum on a CPU gets.  The order depends on the reduction's length alone.
constexpr int NACC = 4;
__device__ __forceinline__ void clear(f32x4 (&acc)[NACC][4]) {
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ float folded(const f32x4 (&acc)[NACC][4], int t, int r) {
    return (acc[0][t][r] + acc[1][t][r]) + (acc[2][t][r] + acc[3][t][r]);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
struct FwdPath {
    const float* in;          // [B,K] (unused with gather)
    const float* w;           // [N,K]
    const float* bias;        // [N]
    float* out;               // [B,N]
    int N, K;
};
struct FwdArgs {
    FwdPath p[MAXP];
    long long B;
    float slope;
    int gather;
    Gather g;
};

__global__ __launch_bounds__(THREADS) void disc_fwd_kernel(FwdArgs a) {
    __shared__ float sa[TILE * LDT], sb[TILE * LDT];
    const int path = blockIdx.z;
    const FwdPath P = a.p[path];
    const int n0 = blockIdx.x * TILE;
    if (n0 >= P.N) return;
    const long long b0 = (long long)blockIdx.y * TILE;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    f32x4 acc[NACC][4];
    clear(acc);
    for (int kq = 0; kq < P.K; kq += NACC * BK) {
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int k0 = kq + q * BK;
            if (k0 >= P.K) continue;                           // (the same for the whole workgroup)
            if (a.gather) {
                const int row = tid >> 2, rq = (tid & 3) * 4;
                const long long b = b0 + row;
#pragma unroll
                for (int c = 0; c < 4; ++c) sa[row * LDT + rq + c] = (b < a.B && k0 + rq + c < P.K) ? gathered(a.g, path, b, k0 + rq + c) : 0.f;
            } else {
                load_r_contig(sa, P.in, (size_t)P.K, b0, a.B, k0, P.K, tid);
            }
            load_r_contig(sb, P.w, (size_t)P.K, n0, P.N, k0, P.K, tid);
            __syncthreads();
            mma_chunk(sa, sb, w, l15, l4, acc[q]);
            __syncthreads();
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + l15;
        if (n >= P.N) continue;
        const float bias = P.bias[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long b = b0 + 16 * w + 4 * l4 + r;
            if (b >= a.B) continue;
            const float z = folded(acc, t, r) + bias;
            P.out[(size_t)b * P.N + n] = z > 0.f ? z : z * a.slope;
        }
    }
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct HeadArgs {
    const float* h[MAXP];     // [B,mid]
    const float* w[MAXP];     // [mid]
    const float* bias[MAXP];  // [1]
    int mid[MAXP];
    long long B;
    int n_paths;
    float* pred;              // [B,n_paths]
};

__global__ __launch_bounds__(THREADS) void disc_head_kernel(HeadArgs a) {
    const int path = blockIdx.y, lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;                                      // (whole waves)
    const int K = a.mid[path];
    const float* h = a.h[path] + (size_t)b * K;
    const float* wv = a.w[path];
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(h[k], wv[k], acc);
    acc = wave_sum_f32(acc);
    if (lane == 0) a.pred[(size_t)b * a.n_paths + path] = acc + a.bias[path][0];
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
struct BwdPath {
    const float* dz;          // [B,N] with row stride ldz (the head: d_pred + path, ldz = n_paths, N = 1)
    const float* w;           // [N,K]
    const float* hprev;       // [B,K]: the tape of the layer below (data: its mask; weight: the other operand); null = layer 1
    float* out;               // data: dH_prev masked [B,K]
    float* dw;                // weight: [N,K] or null
    float* db;                // weight: [N] or null
    int ldz, N, K;
};
struct BwdArgs {
    BwdPath p[MAXP];
    long long B;
    float slope;
    Gather g;                 // weight, layer 1: the other operand
};

__global__ __launch_bounds__(THREADS) void disc_bwd_data_kernel(BwdArgs a) {
    __shared__ float sa[TILE * LDT], sb[TILE * LDT];
    const int path = blockIdx.z;
    const BwdPath P = a.p[path];
    const int k0 = blockIdx.x * TILE;
    if (k0 >= P.K) return;
    const long long b0 = (long long)blockIdx.y * TILE;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    f32x4 acc[NACC][4];
    clear(acc);
    for (int nq = 0; nq < P.N; nq += NACC * BK) {
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int n0 = nq + q * BK;
            if (n0 >= P.N) continue;                           // (the same for the whole workgroup)
            load_r_contig(sa, P.dz, (size_t)P.ldz, b0, a.B, n0, P.N, tid);
            load_j_contig(sb, P.w, (size_t)P.K, k0, P.K, n0, P.N, tid);
            __syncthreads();
            mma_chunk(sa, sb, w, l15, l4, acc[q]);
            __syncthreads();
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int k = k0 + 16 * t + l15;
        if (k >= P.K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long b = b0 + 16 * w + 4 * l4 + r;
            if (b >= a.B) continue;
            const size_t at = (size_t)b * P.K + k;
            float v = folded(acc, t, r);
            if (P.hprev) v *= P.hprev[at] > 0.f ? 1.f : a.slope;
            P.out[at] = v;
        }
    }
}

__global__ __launch_bounds__(THREADS) void disc_bwd_weight_kernel(BwdArgs a) {
    __shared__ float sa[TILE * LDT], sb[TILE * LDT];
    const int path = blockIdx.z;
    const BwdPath P = a.p[path];
    const int k0 = blockIdx.x * TILE, n0 = blockIdx.y * TILE;
    const bool bias_too = blockIdx.x == 0 && P.db;
    if (k0 >= P.K || n0 >= P.N || (!P.dw && !bias_too)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    f32x4 acc[4];
    float tot[4][4];                                         // (scalars: a vector sum would become packed-f32 adds beside the MFMAs)
    double tot_b = 0.0, acc_b = 0.0;                         // threads 0 .. 63 of a column-tile-0 workgroup: column n0 + tid of dZ, in double
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[t][r] = 0.f;
    }
    for (long long c0 = 0; c0 < a.B; c0 += ROW_CHUNK) {
        const long long c1 = c0 + ROW_CHUNK < a.B ? c0 + ROW_CHUNK : a.B;
        for (long long r0 = c0; r0 < c1; r0 += BK) {
            load_j_contig(sa, P.dz, (size_t)P.ldz, n0, P.N, r0, c1, tid);
            if (P.hprev) {
                load_j_contig(sb, P.hprev, (size_t)P.K, k0, P.K, r0, c1, tid);
            } else {
                const int j = tid & 63, rq = tid >> 6;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const long long b = r0 + rq + 4 * c;
                    sb[j * LDT + rq + 4 * c] = (k0 + j < P.K && b < c1) ? gathered(a.g, path, b, k0 + j) : 0.f;
                }
            }
            __syncthreads();
            mma_chunk(sa, sb, w, l15, l4, acc);
            if (bias_too && tid < TILE) {
#pragma unroll
                for (int r = 0; r < BK; ++r) acc_b += (double)sa[tid * LDT + r];
            }
            __syncthreads();
        }
        // the chunk's partial joins the running sum, chunks in order
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) tot[t][r] += acc[t][r];
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        tot_b += acc_b;
        acc_b = 0.0;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n0 + 16 * w + 4 * l4 + r;
        if (n >= P.N) continue;
        if (P.dw) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = k0 + 16 * t + l15;
                if (k < P.K) P.dw[(size_t)n * P.K + k] = tot[t][r];
            }
        }
    }
    if (bias_too && tid < TILE && n0 + tid < P.N) P.db[n0 + tid] = (float)tot_b;
}

struct DxArgs {
    const float* dh0[MAXP];   // [B, n_sel point_dim]
    int n_sel[MAXP];
    int n_paths;
    long long B;
    Gather g;                 // (x unused)
    float* d_x;               // [B,n_points,point_dim]
};

__global__ __launch_bounds__(THREADS) void disc_dx_kernel(DxArgs a) {
    const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int row = a.g.n_points * a.g.point_dim;
    if (idx >= a.B * row) return;
    const long long b = idx / row;
    const int e = (int)(idx - b * row), j = e / a.g.point_dim, c = e - j * a.g.point_dim;
    float sum = 0.f;
    for (int p = 0; p < a.n_paths; ++p) {
        const int ns = a.n_sel[p];
        const float* d = a.dh0[p] + (size_t)b * ns * a.g.point_dim;
        for (int i = 0; i < ns; ++i)
            if (a.g.sel[p][i] == j) sum += d[i * a.g.point_dim + c];
    }
    a.d_x[idx] = sum;
}

// ---- loss --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void disc_loss_kernel(const float* __restrict__ pred, long long n, float label, double weight,
                                                           double* __restrict__ out, float* __restrict__ d_pred) {
    __shared__ double ss[THREADS];
    __shared__ unsigned long long sc[THREADS];
    const int tid = threadIdx.x;
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (long long i = tid; i < n; i += THREADS) {
        const float p = pred[i];
        const double d = (double)p - (double)label;
        sum += d * d;
        cnt += fabsf(p - label) <= 0.5f ? 1u : 0u;
        if (d_pred) d_pred[i] = (float)(weight * 2.0 * d / (double)n);
    }
    ss[tid] = sum;
    sc[tid] = cnt;
    __syncthreads();
    for (int m = THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) { ss[tid] += ss[tid + m]; sc[tid] += sc[tid + m]; }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = weight * (ss[0] / (double)n);
        out[1] = (double)sc[0];
        out[2] = (double)n;
    }
}

// ---- the pool ----------------------------------------------------------------------------------------------------------------------------
struct PoolArgs {
    float* pool;
    const float* items;
    const uint8_t* swap;
    const int32_t* slot;
    float* out;
    long long cap, cur;
    int n, row;
};

// the largest j in [lo, hi) whose (effective) draw swaps into slot s, or -1; every thread of the workgroup receives it
__device__ __forceinline__ int last_swapper(const int32_t* s_slot, int s, int lo, int hi, int* red) {
    int best = -1;
    for (int j = lo + (int)threadIdx.x; j < hi; j += THREADS)
        if (s_slot[j] == s) best = j;                        // (j ascends: the last match stays)
    red[threadIdx.x] = best;
    __syncthreads();
    for (int m = THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + m]);
        __syncthreads();
    }
    const int r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(THREADS) void pool_exchange_kernel(PoolArgs a) {
    extern __shared__ int32_t s_slot[];                       // the items' effective slots: -1 = no swap
    __shared__ int red[THREADS];
    const int i = blockIdx.x, tid = threadIdx.x;
    const long long room = a.cap - a.cur;
    const int n_app = (int)(room < a.n ? room : a.n);         // items 0 .. n_app - 1 are appended
    for (int j = tid; j < a.n; j += THREADS) {
        int s = -1;
        if (j >= n_app && a.swap[j]) {
            s = a.slot[j];
            if (s < 0 || s >= a.cap) s = -1;
        }
        s_slot[j] = s;
    }
    __syncthreads();
    const float* mine = a.items + (size_t)i * a.row;
    float* o = a.out + (size_t)i * a.row;
    if (i < n_app) {
        // appended and returned; the row keeps the last item of this call that swaps into it, if any
        const int s = (int)(a.cur + i);
        const int last = last_swapper(s_slot, s, n_app, a.n, red);
        const float* keep = last >= 0 ? a.items + (size_t)last * a.row : mine;
        float* prow = a.pool + (size_t)s * a.row;
        for (int e = tid; e < a.row; e += THREADS) { o[e] = mine[e]; prow[e] = keep[e]; }
        return;
    }
    const int s = s_slot[i];
    if (s < 0) {
        for (int e = tid; e < a.row; e += THREADS) o[e] = mine[e];
        return;
    }
    const int prev = last_swapper(s_slot, s, n_app, i, red);
    if (prev >= 0) {
        const float* src = a.items + (size_t)prev * a.row;
        for (int e = tid; e < a.row; e += THREADS) o[e] = src[e];
    } else if (s >= a.cur && s < a.cur + n_app) {
        const float* src = a.items + (size_t)(s - a.cur) * a.row;     // a row this call appended (its workgroup writes the pool)
        for (int e = tid; e < a.row; e += THREADS) o[e] = src[e];
    } else {
        // the first swap into an old row: this workgroup alone reads the row and then writes what the call leaves in it
        const int last = last_swapper(s_slot, s, i, a.n, red);
        const float* keep = a.items + (size_t)last * a.row;
        float* prow = a.pool + (size_t)s * a.row;
        for (int e = tid; e < a.row; e += THREADS) { o[e] = prow[e]; prow[e] = keep[e]; }
    }
}

}  // namespace pgdc

// ---- the host side -----------------------------------------------------------------------------------------------------------------------
namespace {

using namespace pgdc;

// the backward's layer gradients and, for a forward without a tape, the activations: grow-only, one set per handle (calls on one
// handle are serialised by the caller)
struct DiscState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_DISC;
    ~DiscState() override { pg_release(act); pg_release(dz[0]); pg_release(dz[1]); pg_release(dh0); }
    DevBuf act, dz[2], dh0;
};

const char* spec_fault(const pg_disc_spec* s) {
    if (!s) return "a null spec";
    if (s->n_paths < 1 || s->n_paths > MAXP) return "n_paths outside [1, 8]";
    if (s->n_points < 1 || s->n_points > MAXS) return "n_points outside [1, 24]";
    if (s->point_dim != 2 && s->point_dim != 3) return "point_dim is neither 2 nor 3";
    // (the backward reads LeakyReLU's mask off the tape's sign: with a negative slope a negative pre-activation leaves a positive tape)
    if (!(s->slope >= 0.f) || isinf(s->slope)) return "slope is negative or not finite";
    for (int p = 0; p < s->n_paths; ++p) {
        const pg_disc_path& q = s->path[p];
        if (q.n_sel < 1 || q.n_sel > s->n_points) return "a path's n_sel outside [1, n_points]";
        if (q.width < 1 || q.mid < 1 || q.width > (1 << 20) || q.mid > (1 << 20)) return "a path's width or mid outside [1, 2^20]";
        for (int i = 0; i < q.n_sel; ++i)
            if (q.sel[i] < 0 || q.sel[i] >= s->n_points) return "a selected row outside [0, n_points)";
    }
    return nullptr;
}

int path_maxdim(const pg_disc_path& q) { return q.width > q.mid ? q.width : q.mid; }
int64_t path_tape(const pg_disc_path& q) { return 3 * (int64_t)q.width + q.mid; }

Gather gather_of(const pg_disc_spec& s, const float* x) {
    Gather g{};
    g.x = x; g.n_points = s.n_points; g.point_dim = s.point_dim;
    for (int p = 0; p < s.n_paths; ++p)
        for (int i = 0; i < s.path[p].n_sel; ++i) g.sel[p][i] = (int8_t)s.path[p].sel[i];
    return g;
}

// the tape's four layers of path p (h[0 .. 3]) in a tape over B rows
void tape_layers(const pg_disc_spec& s, int64_t B, const float* tape, int p, const float* (&h)[4]) {
    const float* at = tape;
    for (int q = 0; q < p; ++q) at += B * path_tape(s.path[q]);
    for (int l = 0; l < 4; ++l) { h[l] = at; at += B * s.path[p].width; }
}

int check_call(pg_handle* h, const char* who, const pg_disc_spec* spec, const pg_disc_params* params, const float* x, int64_t B) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (const char* f = spec_fault(spec)) return pg_fail(h, PG_EINVAL, "%s: %s", who, f);
    if (!params || !x) return pg_fail(h, PG_EINVAL, "%s: params and x are required", who);
    if (B < 1 || B > (int64_t)TILE * 65535) return pg_fail(h, PG_EINVAL, "%s: B = %lld is outside [1, %lld]", who, (long long)B, (long long)TILE * 65535);
    if (pg_misaligned(x, sizeof(float))) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    for (int p = 0; p < spec->n_paths; ++p)
        for (int l = 0; l < PG_DISC_LAYERS; ++l)
            if (!params->w[p][l] || !params->b[p][l] || pg_misaligned(params->w[p][l], sizeof(float)) || pg_misaligned(params->b[p][l], sizeof(float)))
                return pg_fail(h, PG_EINVAL, "%s: path %d, layer %d: a parameter pointer is null or misaligned", who, p, l);
    return PG_OK;
}

unsigned tiles(int64_t n) { return (unsigned)((n + TILE - 1) / TILE); }

}  // namespace

extern "C" int pg_disc_tape_floats(const pg_disc_spec* spec, int64_t B, int64_t* n_floats) {
    if (const char* f = spec_fault(spec)) return pg_fail(nullptr, PG_EINVAL, "pg_disc_tape_floats: %s", f);
    if (B < 1 || !n_floats) return pg_fail(nullptr, PG_EINVAL, "pg_disc_tape_floats: B = %lld, or no place for the result", (long long)B);
    int64_t per_row = 0;
    for (int p = 0; p < spec->n_paths; ++p) per_row += path_tape(spec->path[p]);
    *n_floats = B * per_row;
    return PG_OK;
}

extern "C" int pg_disc_forward(pg_handle* h, void* stream, const pg_disc_spec* spec, const pg_disc_params* params, const float* x, int64_t B,
                               float* pred, float* tape) {
    const char* who = "pg_disc_forward";
    PG_TRY(check_call(h, who, spec, params, x, B));
    if (!pred || pg_misaligned(pred, sizeof(float)) || pg_misaligned(tape, sizeof(float)))
        return pg_fail(h, PG_EINVAL, "%s: pred is required; pred and tape are float arrays", who);
    const pg_disc_spec& s = *spec;
    PG_HIP(h, hipSetDevice(h->device));
    if (!tape) {
        DiscState* st = nullptr;
        PG_TRY(pg_state(h, st));
        int64_t n = 0;
        PG_TRY(pg_disc_tape_floats(spec, B, &n));
        PG_TRY(pg_grow(h, st->act, (size_t)n * sizeof(float), "discriminator activations"));
        tape = st->act.as<float>();
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int max_w = 0, max_m = 0;
    for (int p = 0; p < s.n_paths; ++p) {
        max_w = s.path[p].width > max_w ? s.path[p].width : max_w;
        max_m = s.path[p].mid > max_m ? s.path[p].mid : max_m;
    }
    for (int l = 0; l < 4; ++l) {
        FwdArgs a{};
        a.B = B; a.slope = s.slope; a.gather = l == 0; a.g = gather_of(s, x);
        for (int p = 0; p < s.n_paths; ++p) {
            const float* hl[4];
            tape_layers(s, B, tape, p, hl);
            const pg_disc_path& q = s.path[p];
            a.p[p] = FwdPath{l ? hl[l - 1] : nullptr, params->w[p][l], params->b[p][l], const_cast<float*>(hl[l]), l == 3 ? q.mid : q.width,
                             l ? q.width : q.n_sel * s.point_dim};
        }
        hipLaunchKernelGGL(disc_fwd_kernel, dim3(tiles(l == 3 ? max_m : max_w), tiles(B), (unsigned)s.n_paths), dim3(THREADS), 0, st, a);
        PG_LAUNCH_CHECK(h, "discriminator layer kernel");
    }
    HeadArgs ha{};
    ha.B = B; ha.n_paths = s.n_paths; ha.pred = pred;
    for (int p = 0; p < s.n_paths; ++p) {
        const float* hl[4];
        tape_layers(s, B, tape, p, hl);
        ha.h[p] = hl[3]; ha.w[p] = params->w[p][4]; ha.bias[p] = params->b[p][4]; ha.mid[p] = s.path[p].mid;
    }
    hipLaunchKernelGGL(disc_head_kernel, dim3((unsigned)((B + THREADS / 64 - 1) / (THREADS / 64)), (unsigned)s.n_paths), dim3(THREADS), 0, st, ha);
    PG_LAUNCH_CHECK(h, "discriminator head kernel");
    return PG_OK;
}

extern "C" int pg_disc_backward(pg_handle* h, void* stream, const pg_disc_spec* spec, const pg_disc_params* params, const float* x, int64_t B,
                                const float* tape, const float* d_pred, float* d_x, const pg_disc_grads* grads) {
    const char* who = "pg_disc_backward";
    PG_TRY(check_call(h, who, spec, params, x, B));
    if (!tape || !d_pred || pg_misaligned(tape, sizeof(float)) || pg_misaligned(d_pred, sizeof(float)) || pg_misaligned(d_x, sizeof(float)))
        return pg_fail(h, PG_EINVAL, "%s: tape and d_pred are required; tape, d_pred and d_x are float arrays", who);
    const pg_disc_spec& s = *spec;
    if (grads)
        for (int p = 0; p < s.n_paths; ++p)
            for (int l = 0; l < PG_DISC_LAYERS; ++l)
                if (pg_misaligned(grads->w[p][l], sizeof(float)) || pg_misaligned(grads->b[p][l], sizeof(float)))
                    return pg_fail(h, PG_EINVAL, "%s: path %d, layer %d: a gradient pointer is misaligned", who, p, l);
    DiscState* ws = nullptr;
    PG_TRY(pg_state(h, ws));
    PG_HIP(h, hipSetDevice(h->device));
    int64_t dz_floats = 0, dh0_floats = 0;
    int64_t dz_off[MAXP], dh0_off[MAXP];
    for (int p = 0; p < s.n_paths; ++p) {
        dz_off[p] = dz_floats; dh0_off[p] = dh0_floats;
        dz_floats += B * path_maxdim(s.path[p]);
        dh0_floats += B * s.path[p].n_sel * s.point_dim;
    }
    PG_TRY(pg_grow(h, ws->dz[0], (size_t)dz_floats * sizeof(float), "discriminator layer gradients"));
    PG_TRY(pg_grow(h, ws->dz[1], (size_t)dz_floats * sizeof(float), "discriminator layer gradients"));
    if (d_x) PG_TRY(pg_grow(h, ws->dh0, (size_t)dh0_floats * sizeof(float), "discriminator input gradients"));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Gather g = gather_of(s, x);

    // layer l = 4 (the head) .. 0: dZ of the layer is in `from` (the head: d_pred itself)
    for (int l = 4; l >= 0; --l) {
        BwdArgs a{};
        a.B = B; a.slope = s.slope; a.g = g;
        bool any_grad = false;
        int max_n = 0, max_k = 0;
        float* to = ws->dz[l & 1].as<float>();
        const float* from = ws->dz[(l + 1) & 1].as<float>();
        for (int p = 0; p < s.n_paths; ++p) {
            const float* hl[4];
            tape_layers(s, B, tape, p, hl);
            const pg_disc_path& q = s.path[p];
            BwdPath& P = a.p[p];
            P.N = l == 4 ? 1 : l == 3 ? q.mid : q.width;
            P.K = l == 4 ? q.mid : l == 0 ? q.n_sel * s.point_dim : q.width;
            P.dz = l == 4 ? d_pred + p : from + dz_off[p];
            P.ldz = l == 4 ? s.n_paths : P.N;
            P.w = params->w[p][l];
            P.hprev = l ? hl[l - 1] : nullptr;
            P.out = l ? to + dz_off[p] : (d_x ? ws->dh0.as<float>() + dh0_off[p] : nullptr);
            P.dw = grads ? grads->w[p][l] : nullptr;
            P.db = grads ? grads->b[p][l] : nullptr;
            any_grad = any_grad || P.dw || P.db;
            max_n = P.N > max_n ? P.N : max_n;
            max_k = P.K > max_k ? P.K : max_k;
        }
        if (any_grad) {
            hipLaunchKernelGGL(disc_bwd_weight_kernel, dim3(tiles(max_k), tiles(max_n), (unsigned)s.n_paths), dim3(THREADS), 0, st, a);
            PG_LAUNCH_CHECK(h, "discriminator weight-gradient kernel");
        }
        if (l || d_x) {
            hipLaunchKernelGGL(disc_bwd_data_kernel, dim3(tiles(max_k), tiles(B), (unsigned)s.n_paths), dim3(THREADS), 0, st, a);
            PG_LAUNCH_CHECK(h, "discriminator data-gradient kernel");
        }
    }
    if (d_x) {
        DxArgs da{};
        da.n_paths = s.n_paths; da.B = B; da.g = g; da.d_x = d_x;
        for (int p = 0; p < s.n_paths; ++p) { da.dh0[p] = ws->dh0.as<float>() + dh0_off[p]; da.n_sel[p] = s.path[p].n_sel; }
        const int64_t n = B * s.n_points * s.point_dim;
        hipLaunchKernelGGL(disc_dx_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, da);
        PG_LAUNCH_CHECK(h, "discriminator input-gradient kernel");
    }
    return PG_OK;
}

extern "C" int pg_disc_loss(pg_handle* h, void* stream, const float* pred, int64_t n, float label, double weight, double* out, float* d_pred) {
    const char* who = "pg_disc_loss";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!pred || !out) return pg_fail(h, PG_EINVAL, "%s: pred and out are required", who);
    if (n < 1) return pg_fail(h, PG_EINVAL, "%s: n = %lld", who, (long long)n);
    if (!(label == label) || !(weight == weight)) return pg_fail(h, PG_EINVAL, "%s: the label or the weight is NaN", who);
    if (pg_misaligned(pred, sizeof(float)) || pg_misaligned(d_pred, sizeof(float)) || pg_misaligned(out, sizeof(double)))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    PG_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(disc_loss_kernel, dim3(1), dim3(THREADS), 0, static_cast<hipStream_t>(stream), pred, (long long)n, label, weight, out, d_pred);
    PG_LAUNCH_CHECK(h, "discriminator loss kernel");
    return PG_OK;
}

extern "C" int pg_pool_exchange(pg_handle* h, void* stream, float* pool, int64_t cap, int32_t row_floats, int64_t cur, const float* items, int64_t n,
                                const uint8_t* swap, const int32_t* slot, float* out) {
    const char* who = "pg_pool_exchange";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!pool || !items || !swap || !slot || !out) return pg_fail(h, PG_EINVAL, "%s: pool, items, swap, slot and out are required", who);
    if (cap < 1 || cap > INT32_MAX || row_floats < 1 || cur < 0 || cur > cap)
        return pg_fail(h, PG_EINVAL, "%s: cap = %lld, row_floats = %d, cur = %lld", who, (long long)cap, row_floats, (long long)cur);
    if (n < 1 || n > POOL_MAX_ITEMS) return pg_fail(h, PG_EINVAL, "%s: n = %lld is outside [1, %d]", who, (long long)n, POOL_MAX_ITEMS);
    if (pg_misaligned(pool, sizeof(float)) || pg_misaligned(items, sizeof(float)) || pg_misaligned(out, sizeof(float)) || pg_misaligned(slot, sizeof(int32_t)))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    PG_HIP(h, hipSetDevice(h->device));
    PoolArgs a{pool, items, swap, slot, out, (long long)cap, (long long)cur, (int)n, row_floats};
    hipLaunchKernelGGL(pool_exchange_kernel, dim3((unsigned)n), dim3(THREADS), (size_t)n * sizeof(int32_t), static_cast<hipStream_t>(stream), a);
    PG_LAUNCH_CHECK(h, "pool exchange kernel");
    return PG_OK;
}
