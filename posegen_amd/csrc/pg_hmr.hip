// pg_hmr.hip -- the regression head of the SPIN / HMR regressor on the device (include/posegen_regressor.h): the
// iterative fc stack of HMR.forward (run_gan.py:1343-1356) and rot6d_to_rotmat (:1188-1202), forward and backward.  A chain of small
// float32 GEMMs at B = 20 .. 128 with K up to 2048; nothing couples the rows, so the products are tiled over rows and columns.
//   hmr_gemm_kernel<false> : out = epilogue(A W^T): a wave owns a 16 x 16 tile of the result and walks K in chunks of 16 round four
//                         accumulators on v_mfma_f32_16x16x4_f32 (pg_gen.hip's discipline: chunk c into accumulator c % 4, the four
//                         added as a tree), both operands straight from memory, 16 bytes a lane where the address allows it -- the
//                         [16, K] weight slab of pg_gen.hip does not fit LDS at K = 2048 and is not needed: a workgroup's four waves
//                         share their A rows through the cache, and the row tiles of a column strip share the weights there.
//                         Epilogue: + bias, + a residual operand (P, or the state), dropout mask and scale.
//   hmr_gemm_kernel<true>  : the same with W read down its columns (out = A W): the backward's data products.
//   hmr_wgrad_kernel    : every weight gradient, d_fc1_w's two column ranges and d_xf in one grouped launch: C[n][k] = sum_r A[r][n]
//                         B[r][k] over the stacked rows (gen_wgrad_kernel's 64 x 64 tile and 64-row chunk fold), A with strides and,
//                         for D = sum_i dz1_i, summed in round order on load; bias gradients in double.
//   hmr_init_kernel, hmr_rot_kernel, hmr_rot_bwd_kernel : the state before round 0; the rotation epilogue; its autograd.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/posegen_regressor.h"
#include "pg_handle.h"

namespace pghm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WAVES = 4, THREADS = 64 * WAVES;      // the product kernel: four 16 x 16 tiles side by side
constexpr int NACC = 4;                             // accumulators a reduction goes round, chunk c into c % 4 (as pg_disc.hip, pg_gen.hip)
constexpr int KSTEP = 16 * NACC;
constexpr double NORM_EPS = 1e-12;                  // F.normalize's eps

// Rows of up to three tensors laid end to end (the decoders), or of one (n1 = n2 = its rows): row r starts at p[.] + r' ld + off.
struct Rows {
    const float* p[3];
    int n1, n2;
    long long ld;
    int off;
};
__device__ __forceinline__ int segment_of(int n1, int n2, int r, int& rr) {
    if (r < n1) { rr = r; return 0; }
    if (r < n2) { rr = r - n1; return 1; }
    rr = r - n2;
    return 2;
}
// entry s of a three-pointer table by selects (an index that is not a constant would put the table in scratch memory)
template <class T> __device__ __forceinline__ T pick3(T const (&p)[3], int s) { return s == 0 ? p[0] : (s == 1 ? p[1] : p[2]); }
__device__ __forceinline__ const float* row_of(const Rows& w, int r) {
    int rr;
    const int s = segment_of(w.n1, w.n2, r, rr);
    return pick3(w.p, s) + (size_t)rr * w.ld + w.off;
}

// values k .. k + 3 of a row (zero past K and for a null row): one 16-byte load where the address allows it, else element by
// element -- the same values either way
__device__ __forceinline__ void load4(const float* row, int k, int K, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (!row || k >= K) return;
    const float* p = row + k;
    if (k + 3 < K && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) if (k + c < K) v[c] = p[c];
    }
}

struct GemmArgs {
    const float* a;           // [M,K], row stride lda
    long long lda;
    Rows w;                   // <false>: row n of W, k along it; <true>: row k of W, n along it
    const float* bias[3];     // [N] in the segments of w (<false> only); null = none
    const float* add;         // [M,N], row stride ldadd: out = add + (c + bias); null = none
    long long ldadd;
    const unsigned char* mask;   // [M,N] non-zero = kept; null = no dropout
    float scale;              // fl32(1 / (1 - p))
    float* out;               // [M,N], row stride ldo
    long long ldo;
    long long M;
    int N, K;
};

// Lane (l15, l4) supplies k = 16 c + 4 l4 + s to step s of chunk c for both operands; the result's lane holds rows 4 l4 .. 4 l4 + 3 of
// column l15.  Chunk c goes into accumulator c % 4 and the four are added as a tree: an order that depends on K alone.
template <bool NN>
__global__ __launch_bounds__(THREADS) void hmr_gemm_kernel(GemmArgs g) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const long long row0 = (long long)blockIdx.x * 16;
    const int n0 = ((int)blockIdx.y * WAVES + wv) * 16;
    if (n0 >= g.N) return;                                      // (the whole wave)
    const int N = g.N, K = g.K, n = n0 + l15;
    const long long ar = row0 + l15;
    const float* arow = ar < g.M ? g.a + (size_t)ar * g.lda : nullptr;
    const float* wrow = (!NN && n < N) ? row_of(g.w, n) : nullptr;
    f32x4 acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kq = 0; kq < K; kq += KSTEP) {
        float a[NACC][4], w[NACC][4];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int k = kq + 16 * q + 4 * l4;
            load4(arow, k, K, a[q]);
            if (!NN) {
                load4(wrow, k, K, w[q]);
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) w[q][s] = (k + s < K && n < N) ? row_of(g.w, k + s)[n] : 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < NACC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][s], w[q][s], acc[q], 0, 0, 0);
    }
    if (n >= N) return;
    float bias = 0.f;
    bool has_bias = false;
    if (!NN) {
        int rr;
        const int sg = segment_of(g.w.n1, g.w.n2, n, rr);
        const float* bp = pick3(g.bias, sg);
        if (bp) { bias = bp[rr]; has_bias = true; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long b = row0 + 4 * l4 + r;
        if (b >= g.M) continue;
        float v = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
        if (has_bias) v = v + bias;
        if (g.add) v = g.add[(size_t)b * g.ldadd + n] + v;
        if (g.mask) v = g.mask[(size_t)b * N + n] ? v * g.scale : 0.f;
        g.out[(size_t)b * g.ldo + n] = v;
    }
}

// ---- weight gradients, d_xf ----------------------------------------------------------------------------------------------------------
constexpr int WT = 64, WTHREADS = 256, BK = 16, LDT = BK + 1, ROW_CHUNK = 64;   // gen_wgrad_kernel's tile and chunk fold
constexpr int MAXG = 5;

// C[n][k] = sum over rounds i and rows r of A_i[r][n] B_i[r][k]
struct WGroup {
    const float* a;           // A_i[r][n] at a + i a_round + r a_sr + n a_sn
    long long a_sr, a_sn, a_round;
    int a_sum;                // > 0: one round whose A is the sum of a_sum arrays a_round apart, added in order as it is loaded
    const float* b;           // B_i[r][k] at b + i b_round + r b_sr + k
    long long b_sr, b_round;
    float* c[3];              // rows of C in the segments n1, n2 (as Rows); a null segment is not written
    float* cb[3];             // column sums of A over all stacked rows, in double; null = not wanted
    int n1, n2;
    long long ldc;
    int coff;                 // C's first column
    int N, K, rounds;
    long long R;              // rows of a round
};
struct WArgs {
    WGroup g[MAXG];
};

__global__ __launch_bounds__(WTHREADS) void hmr_wgrad_kernel(WArgs args) {
    __shared__ float sa[WT * LDT], sb[WT * LDT];
    const WGroup P = args.g[blockIdx.z];
    const int k0 = blockIdx.x * WT, n0 = blockIdx.y * WT;
    const bool any_c = P.c[0] || P.c[1] || P.c[2];
    const bool bias_too = blockIdx.x == 0 && (P.cb[0] || P.cb[1] || P.cb[2]);
    if (k0 >= P.K || n0 >= P.N || (!any_c && !bias_too)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int j = tid & 63, rq = tid >> 6;
    f32x4 acc[4];
    float tot[4][4];                                         // (scalars: a vector sum would become packed-f32 adds beside the MFMAs)
    double tot_b = 0.0, acc_b = 0.0;                         // threads 0 .. 63 of a column-tile-0 workgroup: column n0 + tid of A, in double
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[t][r] = 0.f;
    }
    for (int i = 0; i < P.rounds; ++i) {
        const float* A = P.a + (size_t)i * P.a_round;
        const float* Bm = P.b + (size_t)i * P.b_round;
        for (long long c0 = 0; c0 < P.R; c0 += ROW_CHUNK) {
            const long long c1 = c0 + ROW_CHUNK < P.R ? c0 + ROW_CHUNK : P.R;
            for (long long r0 = c0; r0 < c1; r0 += BK) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const long long b = r0 + rq + 4 * c;
                    float va = 0.f, vb = 0.f;
                    if (n0 + j < P.N && b < c1) {
                        const float* p = A + (size_t)b * P.a_sr + (size_t)(n0 + j) * P.a_sn;
                        va = p[0];
                        for (int q = 1; q < P.a_sum; ++q) va += p[(size_t)q * P.a_round];
                    }
                    if (k0 + j < P.K && b < c1) vb = Bm[(size_t)b * P.b_sr + k0 + j];
                    sa[j * LDT + rq + 4 * c] = va;
                    sb[j * LDT + rq + 4 * c] = vb;
                }
                __syncthreads();
#pragma unroll
                for (int s = 0; s < BK / 4; ++s) {
                    const float av = sa[(16 * w + l15) * LDT + 4 * s + l4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sb[(16 * t + l15) * LDT + 4 * s + l4], acc[t], 0, 0, 0);
                }
                if (bias_too && tid < WT) {
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
    }
    if (any_c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 16 * w + 4 * l4 + r;
            if (n >= P.N) continue;
            int rr;
            float* crow = pick3(P.c, segment_of(P.n1, P.n2, n, rr));
            if (!crow) continue;
            crow += (size_t)rr * P.ldc + P.coff;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = k0 + 16 * t + l15;
                if (k < P.K) crow[k] = tot[t][r];
            }
        }
    }
    if (bias_too && tid < WT && n0 + tid < P.N) {
        int rr;
        float* cb = pick3(P.cb, segment_of(P.n1, P.n2, n0 + tid, rr));
        if (cb) cb[rr] = (float)tot_b;
    }
}

// ---- the state before round 0 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hmr_init_kernel(const float* __restrict__ init, int per_row, long long B, int S, float* __restrict__ s0) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * S) return;
    s0[i] = per_row ? init[i] : init[i % S];
}

// ---- the rotation epilogue -----------------------------------------------------------------------------------------------------------------
// one thread per (row, unit): a unit is a joint (six state columns -> nine numbers) or one shape / cam column (copied)
__global__ __launch_bounds__(256) void hmr_rot_kernel(const float* __restrict__ s, long long B, int J, int n_shape, int n_cam,
                                                      float* __restrict__ rotmat, float* __restrict__ shape, float* __restrict__ cam) {
    const int U = J + n_shape + n_cam, S = 6 * J + n_shape + n_cam;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * U) return;
    const long long b = i / U;
    const int u = (int)(i - b * U);
    const float* row = s + (size_t)b * S;
    if (u >= J) {
        const int c = u - J;
        if (c < n_shape) { if (shape) shape[(size_t)b * n_shape + c] = row[6 * J + c]; }
        else if (cam) cam[(size_t)b * n_cam + (c - n_shape)] = row[6 * J + c];
        return;
    }
    if (!rotmat) return;
    const float* x = row + 6 * u;
    const double a1[3] = {x[0], x[2], x[4]}, a2[3] = {x[1], x[3], x[5]};
    const double c1 = fmax(sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), NORM_EPS);
    const double b1[3] = {a1[0] / c1, a1[1] / c1, a1[2] / c1};
    const double d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const double v[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const double c2 = fmax(sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), NORM_EPS);
    const double b2[3] = {v[0] / c2, v[1] / c2, v[2] / c2};
    const double b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
    float* R = rotmat + ((size_t)b * J + u) * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        R[3 * r] = (float)b1[r];
        R[3 * r + 1] = (float)b2[r];
        R[3 * r + 2] = (float)b3[r];
    }
}

// the cotangent of the final state [B,S] from d_rotmat, d_shape and d_cam (a null one = zero): the autograd of the expression above
__global__ __launch_bounds__(256) void hmr_rot_bwd_kernel(const float* __restrict__ s, const float* __restrict__ d_rotmat, const float* __restrict__ d_shape,
                                                          const float* __restrict__ d_cam, long long B, int J, int n_shape, int n_cam,
                                                          float* __restrict__ ds) {
    const int U = J + n_shape + n_cam, S = 6 * J + n_shape + n_cam;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * U) return;
    const long long b = i / U;
    const int u = (int)(i - b * U);
    float* o = ds + (size_t)b * S;
    if (u >= J) {
        const int c = u - J;
        if (c < n_shape) o[6 * J + c] = d_shape ? d_shape[(size_t)b * n_shape + c] : 0.f;
        else o[6 * J + c] = d_cam ? d_cam[(size_t)b * n_cam + (c - n_shape)] : 0.f;
        return;
    }
    o += 6 * u;
    if (!d_rotmat) {
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = 0.f;
        return;
    }
    const float* x = s + (size_t)b * S + 6 * u;
    const float* G = d_rotmat + ((size_t)b * J + u) * 9;
    const double a1[3] = {x[0], x[2], x[4]}, a2[3] = {x[1], x[3], x[5]};
    const double g1[3] = {G[0], G[3], G[6]}, g2[3] = {G[1], G[4], G[7]}, g3[3] = {G[2], G[5], G[8]};
    const double n1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), c1 = fmax(n1, NORM_EPS);
    const double b1[3] = {a1[0] / c1, a1[1] / c1, a1[2] / c1};
    const double d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const double v[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const double n2 = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), c2 = fmax(n2, NORM_EPS);
    const double b2[3] = {v[0] / c2, v[1] / c2, v[2] / c2};
    // b3 = b1 x b2
    double gb1[3] = {g1[0] + (b2[1] * g3[2] - b2[2] * g3[1]), g1[1] + (b2[2] * g3[0] - b2[0] * g3[2]), g1[2] + (b2[0] * g3[1] - b2[1] * g3[0])};
    const double gb2[3] = {g2[0] + (g3[1] * b1[2] - g3[2] * b1[1]), g2[1] + (g3[2] * b1[0] - g3[0] * b1[2]), g2[2] + (g3[0] * b1[1] - g3[1] * b1[0])};
    // b2 = v / max(|v|, eps)
    double gv[3];
    if (n2 >= NORM_EPS) {
        const double t = b2[0] * gb2[0] + b2[1] * gb2[1] + b2[2] * gb2[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) gv[c] = (gb2[c] - b2[c] * t) / n2;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) gv[c] = gb2[c] / NORM_EPS;
    }
    // v = a2 - (b1 . a2) b1
    const double t1 = b1[0] * gv[0] + b1[1] * gv[1] + b1[2] * gv[2];
    double ga2[3], ga1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ga2[c] = gv[c] - b1[c] * t1;
        gb1[c] += -d * gv[c] - a2[c] * t1;
    }
    // b1 = a1 / max(|a1|, eps)
    if (n1 >= NORM_EPS) {
        const double t = b1[0] * gb1[0] + b1[1] * gb1[1] + b1[2] * gb1[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) ga1[c] = (gb1[c] - b1[c] * t) / n1;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) ga1[c] = gb1[c] / NORM_EPS;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[2 * c] = (float)ga1[c];
        o[2 * c + 1] = (float)ga2[c];
    }
}

}  // namespace pghm

// ---- the host side -----------------------------------------------------------------------------------------------------------------------
namespace {

using namespace pghm;

// the backward's d_s, dz2 and dz1 of every round: grow-only, one per handle (calls on one handle are serialised by the caller)
struct HmrState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_HMR;
    ~HmrState() override { pg_release(ws); }
    DevBuf ws;
};

const char* spec_fault(const pg_hmr_spec* s) {
    if (!s) return "a null spec";
    if (s->n_feat < 1 || s->n_feat > PG_HMR_MAX_FEAT) return "n_feat outside [1, 4096]";
    if (s->n_hidden < 1 || s->n_hidden > PG_HMR_MAX_HIDDEN) return "n_hidden outside [1, 2048]";
    if (s->n_joints < 1 || s->n_joints > PG_HMR_MAX_JOINTS) return "n_joints outside [1, 64]";
    if (s->n_shape < 0 || s->n_shape > PG_HMR_MAX_SHAPE) return "n_shape outside [0, 64]";
    if (s->n_cam < 0 || s->n_cam > PG_HMR_MAX_CAM) return "n_cam outside [0, 16]";
    if (s->n_iter < 1 || s->n_iter > PG_HMR_MAX_ITER) return "n_iter outside [1, 8]";
    if (!(s->p_drop >= 0.f && s->p_drop < 1.f)) return "p_drop is not in [0, 1)";
    return nullptr;
}

bool bad_f(const void* p) { return pg_misaligned(p, sizeof(float)); }

struct Dims {
    int64_t B, F, H, S, n;
    int J, n_shape, n_cam;
    int64_t P() const { return 0; }
    int64_t s(int i) const { return B * H + i * B * S; }
    int64_t h1(int i) const { return B * H + (n + 1) * B * S + 2 * i * B * H; }
    int64_t h2(int i) const { return h1(i) + B * H; }
    int64_t end() const { return h1((int)n); }
};
Dims dims_of(const pg_hmr_spec& s, int64_t B) {
    Dims d;
    d.B = B; d.F = s.n_feat; d.H = s.n_hidden; d.J = s.n_joints; d.n_shape = s.n_shape; d.n_cam = s.n_cam; d.n = s.n_iter;
    d.S = 6 * (int64_t)s.n_joints + s.n_shape + s.n_cam;
    return d;
}

int check_common(pg_handle* h, const char* who, const pg_hmr_spec* spec, int64_t B) {
    if (const char* f = spec_fault(spec)) return pg_fail(h, PG_EINVAL, "%s: %s", who, f);
    if (B < 1 || B > PG_HMR_MAX_ROWS) return pg_fail(h, PG_EINVAL, "%s: B = %lld is outside [1, %d]", who, (long long)B, PG_HMR_MAX_ROWS);
    return PG_OK;
}

int check_call(pg_handle* h, const char* who, const pg_hmr_spec* spec, const pg_hmr_params* p, const float* xf, const uint8_t* masks, int64_t B,
               const float* tape) {
    PG_TRY(check_common(h, who, spec, B));
    if (!p || !xf || !tape) return pg_fail(h, PG_EINVAL, "%s: params, xf and tape are required", who);
    if (bad_f(xf) || bad_f(tape)) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    const void* need[6] = {p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->decpose_w, p->decpose_b};
    for (const void* q : need)
        if (!q) return pg_fail(h, PG_EINVAL, "%s: a parameter pointer is null", who);
    if (spec->n_shape && (!p->decshape_w || !p->decshape_b)) return pg_fail(h, PG_EINVAL, "%s: a parameter pointer is null", who);
    if (spec->n_cam && (!p->deccam_w || !p->deccam_b)) return pg_fail(h, PG_EINVAL, "%s: a parameter pointer is null", who);
    const void* all[10] = {p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->decpose_w, p->decpose_b, p->decshape_w, p->decshape_b, p->deccam_w, p->deccam_b};
    for (const void* q : all)
        if (bad_f(q)) return pg_fail(h, PG_EINVAL, "%s: a parameter pointer is misaligned", who);
    return PG_OK;
}

Rows decoders(const pg_hmr_params& p, const Dims& d) {
    return Rows{{p.decpose_w, p.decshape_w, p.deccam_w}, 6 * d.J, 6 * d.J + d.n_shape, d.H, 0};
}
Rows one(const float* w, int rows, long long ld, int off) { return Rows{{w, nullptr, nullptr}, rows, rows, ld, off}; }

template <bool NN> void launch_gemm(hipStream_t st, const GemmArgs& g) {
    const dim3 grid((unsigned)((g.M + 15) / 16), (unsigned)((g.N + 16 * WAVES - 1) / (16 * WAVES)));
    hipLaunchKernelGGL((hmr_gemm_kernel<NN>), grid, dim3(THREADS), 0, st, g);
}

float drop_scale(const pg_hmr_spec& s) { return (float)(1.0 / (1.0 - (double)s.p_drop)); }
unsigned wtiles(int64_t n) { return (unsigned)((n + WT - 1) / WT); }

}  // namespace

extern "C" int pg_hmr_tape_size(const pg_hmr_spec* spec, int64_t B, int64_t* n_floats) {
    PG_TRY(check_common(nullptr, "pg_hmr_tape_size", spec, B));
    if (!n_floats) return pg_fail(nullptr, PG_EINVAL, "pg_hmr_tape_size: no place for the result");
    *n_floats = dims_of(*spec, B).end();
    return PG_OK;
}

extern "C" int pg_hmr_head_forward(pg_handle* h, void* stream, const pg_hmr_spec* spec, const pg_hmr_params* params, const float* xf,
                                   const float* init, int32_t init_per_row, const uint8_t* masks, int64_t B, float* tape, float* rotmat,
                                   float* shape, float* cam) {
    const char* who = "pg_hmr_head_forward";
    PG_TRY(check_call(h, who, spec, params, xf, masks, B, tape));
    if (!init) return pg_fail(h, PG_EINVAL, "%s: init is required", who);
    if (bad_f(init) || bad_f(rotmat) || bad_f(shape) || bad_f(cam)) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    const pg_hmr_params& p = *params;
    const Dims d = dims_of(*spec, B);
    const int F = (int)d.F, H = (int)d.H, S = (int)d.S;
    const float scale = drop_scale(*spec);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(hmr_init_kernel, dim3((unsigned)((B * S + 255) / 256)), dim3(256), 0, st, init, (int)(init_per_row != 0), (long long)B, S,
                       tape + d.s(0));
    PG_LAUNCH_CHECK(h, "regression head state kernel");
    {   // P = xf W1[:, :F]^T + b1
        GemmArgs g{};
        g.a = xf; g.lda = F; g.w = one(p.fc1_w, H, F + S, 0); g.bias[0] = p.fc1_b; g.out = tape + d.P(); g.ldo = H; g.M = B; g.N = H; g.K = F;
        launch_gemm<false>(st, g);
        PG_LAUNCH_CHECK(h, "regression head feature product");
    }
    for (int i = 0; i < d.n; ++i) {
        const uint8_t* m1 = masks ? masks + (size_t)(2 * i) * B * H : nullptr;
        const uint8_t* m2 = masks ? masks + (size_t)(2 * i + 1) * B * H : nullptr;
        GemmArgs g{};
        g.a = tape + d.s(i); g.lda = S; g.w = one(p.fc1_w, H, F + S, F); g.add = tape + d.P(); g.ldadd = H; g.mask = m1; g.scale = scale;
        g.out = tape + d.h1(i); g.ldo = H; g.M = B; g.N = H; g.K = S;
        launch_gemm<false>(st, g);
        PG_LAUNCH_CHECK(h, "regression head fc1 state product");
        g = GemmArgs{};
        g.a = tape + d.h1(i); g.lda = H; g.w = one(p.fc2_w, H, H, 0); g.bias[0] = p.fc2_b; g.mask = m2; g.scale = scale;
        g.out = tape + d.h2(i); g.ldo = H; g.M = B; g.N = H; g.K = H;
        launch_gemm<false>(st, g);
        PG_LAUNCH_CHECK(h, "regression head fc2 product");
        g = GemmArgs{};
        g.a = tape + d.h2(i); g.lda = H; g.w = decoders(p, d); g.bias[0] = p.decpose_b; g.bias[1] = p.decshape_b; g.bias[2] = p.deccam_b;
        g.add = tape + d.s(i); g.ldadd = S; g.out = tape + d.s(i + 1); g.ldo = S; g.M = B; g.N = S; g.K = H;
        launch_gemm<false>(st, g);
        PG_LAUNCH_CHECK(h, "regression head decoder product");
    }
    if (rotmat || shape || cam) {
        const int64_t units = B * (d.J + d.n_shape + d.n_cam);
        hipLaunchKernelGGL(hmr_rot_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, st, tape + d.s((int)d.n), (long long)B, d.J, d.n_shape,
                           d.n_cam, rotmat, shape, cam);
        PG_LAUNCH_CHECK(h, "regression head rotation kernel");
    }
    return PG_OK;
}

extern "C" int pg_hmr_head_backward(pg_handle* h, void* stream, const pg_hmr_spec* spec, const pg_hmr_params* params, const float* xf,
                                    const uint8_t* masks, int64_t B, const float* tape, const float* d_rotmat, const float* d_shape,
                                    const float* d_cam, const pg_hmr_grads* grads, float* d_xf, float* d_init) {
    const char* who = "pg_hmr_head_backward";
    PG_TRY(check_call(h, who, spec, params, xf, masks, B, tape));
    if (!d_rotmat && !(d_shape && spec->n_shape) && !(d_cam && spec->n_cam)) return pg_fail(h, PG_EINVAL, "%s: no cotangent at all", who);
    if (bad_f(d_rotmat) || bad_f(d_shape) || bad_f(d_cam) || bad_f(d_xf) || bad_f(d_init))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    pg_hmr_grads gr{};
    if (grads) gr = *grads;
    {
        const void* all[10] = {gr.fc1_w, gr.fc1_b, gr.fc2_w, gr.fc2_b, gr.decpose_w, gr.decpose_b, gr.decshape_w, gr.decshape_b, gr.deccam_w, gr.deccam_b};
        for (const void* q : all)
            if (bad_f(q)) return pg_fail(h, PG_EINVAL, "%s: a gradient pointer is misaligned", who);
    }
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    const pg_hmr_params& p = *params;
    const Dims d = dims_of(*spec, B);
    const int F = (int)d.F, H = (int)d.H, S = (int)d.S, n = (int)d.n;
    if (!d.n_shape) gr.decshape_w = gr.decshape_b = nullptr;
    if (!d.n_cam) gr.deccam_w = gr.deccam_b = nullptr;
    const float scale = drop_scale(*spec);
    HmrState* state = nullptr;
    PG_TRY(pg_state(h, state));
    PG_HIP(h, hipSetDevice(h->device));
    const int64_t BS = B * S, BH = B * H;
    PG_TRY(pg_grow(h, state->ws, (size_t)((n + 1) * BS + 2 * n * BH) * sizeof(float), "regression head gradients"));
    float* ds = state->ws.as<float>();                 // d_s_k at ds + k BS, k = 0 .. n
    float* dz2 = ds + (n + 1) * BS;                    // round i at dz2 + i BH
    float* dz1 = dz2 + n * BH;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        const int64_t units = B * (d.J + d.n_shape + d.n_cam);
        hipLaunchKernelGGL(hmr_rot_bwd_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, st, tape + d.s(n), d_rotmat, d_shape, d_cam,
                           (long long)B, d.J, d.n_shape, d.n_cam, ds + n * BS);
        PG_LAUNCH_CHECK(h, "regression head rotation backward kernel");
    }
    for (int i = n - 1; i >= 0; --i) {
        const uint8_t* m1 = masks ? masks + (size_t)(2 * i) * B * H : nullptr;
        const uint8_t* m2 = masks ? masks + (size_t)(2 * i + 1) * B * H : nullptr;
        GemmArgs g{};
        g.a = ds + (i + 1) * BS; g.lda = S; g.w = decoders(p, d); g.mask = m2; g.scale = scale; g.out = dz2 + i * BH; g.ldo = H; g.M = B; g.N = H; g.K = S;
        launch_gemm<true>(st, g);
        PG_LAUNCH_CHECK(h, "regression head decoder data gradient");
        g = GemmArgs{};
        g.a = dz2 + i * BH; g.lda = H; g.w = one(p.fc2_w, H, H, 0); g.mask = m1; g.scale = scale; g.out = dz1 + i * BH; g.ldo = H; g.M = B; g.N = H; g.K = H;
        launch_gemm<true>(st, g);
        PG_LAUNCH_CHECK(h, "regression head fc2 data gradient");
        float* out = i ? ds + i * BS : d_init;
        if (!out) continue;
        g = GemmArgs{};
        g.a = dz1 + i * BH; g.lda = H; g.w = one(p.fc1_w, H, F + S, F); g.add = ds + (i + 1) * BS; g.ldadd = S; g.out = out; g.ldo = S; g.M = B; g.N = S; g.K = H;
        launch_gemm<true>(st, g);
        PG_LAUNCH_CHECK(h, "regression head state data gradient");
    }
    WArgs wa{};
    int ng = 0;
    int64_t max_n = 0, max_k = 0;
    auto push = [&](const WGroup& G) {
        wa.g[ng++] = G;
        max_n = G.N > max_n ? G.N : max_n;
        max_k = G.K > max_k ? G.K : max_k;
    };
    if (gr.decpose_w || gr.decpose_b || gr.decshape_w || gr.decshape_b || gr.deccam_w || gr.deccam_b) {
        WGroup G{};
        G.a = ds + BS; G.a_sr = S; G.a_sn = 1; G.a_round = BS; G.b = tape + d.h2(0); G.b_sr = H; G.b_round = 2 * BH;
        G.c[0] = gr.decpose_w; G.c[1] = gr.decshape_w; G.c[2] = gr.deccam_w; G.cb[0] = gr.decpose_b; G.cb[1] = gr.decshape_b; G.cb[2] = gr.deccam_b;
        G.n1 = 6 * d.J; G.n2 = 6 * d.J + d.n_shape; G.ldc = H; G.N = S; G.K = H; G.rounds = n; G.R = B;
        push(G);
    }
    if (gr.fc2_w || gr.fc2_b) {
        WGroup G{};
        G.a = dz2; G.a_sr = H; G.a_sn = 1; G.a_round = BH; G.b = tape + d.h1(0); G.b_sr = H; G.b_round = 2 * BH;
        G.c[0] = gr.fc2_w; G.cb[0] = gr.fc2_b; G.n1 = G.n2 = H; G.ldc = H; G.N = H; G.K = H; G.rounds = n; G.R = B;
        push(G);
    }
    if (gr.fc1_w || gr.fc1_b) {
        WGroup G{};
        G.a = dz1; G.a_sr = H; G.a_sn = 1; G.a_round = BH; G.b = tape + d.s(0); G.b_sr = S; G.b_round = BS;
        G.c[0] = gr.fc1_w; G.cb[0] = gr.fc1_b; G.n1 = G.n2 = H; G.ldc = F + S; G.coff = F; G.N = H; G.K = S; G.rounds = n; G.R = B;
        push(G);
    }
    if (gr.fc1_w) {
        WGroup G{};
        G.a = dz1; G.a_sr = H; G.a_sn = 1; G.a_round = BH; G.a_sum = n; G.b = xf; G.b_sr = F;
        G.c[0] = gr.fc1_w; G.n1 = G.n2 = H; G.ldc = F + S; G.N = H; G.K = F; G.rounds = 1; G.R = B;
        push(G);
    }
    if (d_xf) {
        // d_xf[b][f] = sum_h D[b][h] W1[h][f]: the same product with D read across (A[r = h][n = b])
        WGroup G{};
        G.a = dz1; G.a_sr = 1; G.a_sn = H; G.a_round = BH; G.a_sum = n; G.b = p.fc1_w; G.b_sr = F + S;
        G.c[0] = d_xf; G.n1 = G.n2 = (int)B; G.ldc = F; G.N = (int)B; G.K = F; G.rounds = 1; G.R = H;
        push(G);
    }
    if (ng) {
        hipLaunchKernelGGL(hmr_wgrad_kernel, dim3(wtiles(max_k), wtiles(max_n), (unsigned)ng), dim3(WTHREADS), 0, st, wa);
        PG_LAUNCH_CHECK(h, "regression head weight-gradient kernel");
    }
    return PG_OK;
}
