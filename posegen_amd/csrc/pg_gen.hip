// pg_gen.hip -- the pose generator of the PoseGen loop on the device (include/posegen_generator.h): the noise MLPs of
// BAGenerator / RTGenerator (run_gan.py:767-980), Linear -> BatchNorm1d -> LeakyReLU per layer, forward and backward, and the two heads.
// BatchNorm couples the rows of a batch only within a column, so the workgroup that owns 16 columns walks all B rows and sees all its
// columns' statistics need: no grid-wide reduction, no atomics, no cooperative launch.
//   gen_fwd_kernel<false> : one layer of every trunk in one launch.  A workgroup of 16 waves owns 16 output columns; the [16, K] weight
//                        slab sits in LDS once; wave w takes the row tiles w, w + 16, ...; K in chunks of 16 round four accumulators
//                        on v_mfma_f32_16x16x4_f32, four chunks in flight (four independent accumulators under the 40-cycle dependent
//                        latency).  The operand is the previous layer's activation, formed from its Z, scale and shift on load.  Z
//                        goes to the tape; then the column statistics of the workgroup's own Z in double, two passes.
//   gen_fwd_kernel<true>  : BAGenerator's head on the same tile code, the axis-angle epilogue in place of the statistics.
//   gen_bwd_kernel<true>  : dH = dZ_next W_next[:, tile] (or the cotangent), the mask and x^ from the tape, d_beta and d_gamma in double,
//                        dZ written in place of dY.   <false>: the head's d_h = dy w2, no BatchNorm.
//   gen_wgrad_kernel   : every dW = dZ^T H_prev and db = colsum(dZ) of all layers and trunks in one grouped launch
//                        (disc_bwd_weight_kernel's tile and 64-row chunk fold, H_prev recomputed on load).
//   ba_head_dy_kernel, rt_head_kernel : see the header.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/posegen_generator.h"
#include "pg_handle.h"
#include "pg_kin.h"

namespace pggn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WAVES = 16, THREADS = 64 * WAVES;   // the column-tile kernels
constexpr int TN = 16;                              // columns of a workgroup
constexpr int GROUPS = THREADS / TN;                // row groups of the statistics passes: group g takes rows g, g + 64, ...
constexpr int NACC = 4;                             // accumulators a reduction goes round, chunk c into c % 4 (as pg_disc.hip)
constexpr int KSTEP = 16 * NACC;
constexpr int MAXT = PG_GEN_MAX_TRUNKS, MAXL = PG_GEN_MAX_LAYERS;

__device__ __forceinline__ int padded(int K) { return (K + KSTEP - 1) / KSTEP * KSTEP; }

// the activation of a layer from its tape: the one expression that the forward's next layer, the heads and the backward's mask share
__device__ __forceinline__ float bn_pre(float z, float scale, float shift) { return fmaf(z, scale, shift); }
__device__ __forceinline__ float lrelu(float y, float slope) { return y > 0.f ? y : y * slope; }

// An operand [B, K] with row stride K: as stored, or (sc != null) the activation of the layer whose Z it is.  sc / sh: LDS, zero past K.
struct Operand {
    const float* p;
    const float* sc;
    const float* sh;
    float slope;
};

// values k .. k + 3 of row b (zero past K and past B): one 16-byte load where the address allows it, else element by element --
// the same values either way
__device__ __forceinline__ void load4(const Operand& o, long long b, long long B, int k, int K, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (b >= B || k >= K) return;
    const float* p = o.p + (size_t)b * K + k;
    if (k + 3 < K && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) if (k + c < K) v[c] = p[c];
    }
    if (o.sc) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = lrelu(bn_pre(v[c], o.sc[k + c], o.sh[k + c]), o.slope);   // (zero past K: sc = sh = 0 there)
    }
}

// rows 16 rt .. 16 rt + 15 of the operand against the slab S [16][ld] (row j = output column j, zero past K): the wave's 16 x 16 tile.
// Lane (l15, l4) supplies k = 16 c + 4 l4 + s to step s of chunk c for both operands; chunk c goes into accumulator c % 4 and the
// four are added as a tree: an order that depends on K alone.
__device__ __forceinline__ void tile_product(const Operand& o, const float* S, int ld, long long row0, long long B, int K, int l15, int l4, float (&out)[4]) {
    f32x4 acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int Kp = padded(K);
    for (int kq = 0; kq < Kp; kq += KSTEP) {
        float a[NACC][4];
        f32x4 w[NACC];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            load4(o, row0 + l15, B, kq + 16 * q + 4 * l4, K, a[q]);
            w[q] = *reinterpret_cast<const f32x4*>(S + l15 * ld + kq + 16 * q + 4 * l4);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < NACC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][s], w[q][s], acc[q], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
}

// the LDS of a column-tile kernel: two double arrays for the statistics, the slab, the previous layer's scale and shift
struct Lds {
    double* red0;
    double* red1;
    float* S;
    float* sc;
    float* sh;
    int ld;
};
__device__ __forceinline__ Lds carve_lds(void* base, int K) {
    Lds L;
    L.red0 = reinterpret_cast<double*>(base);
    L.red1 = L.red0 + THREADS;
    L.ld = padded(K) + 4;
    L.S = reinterpret_cast<float*>(L.red1 + THREADS);
    L.sc = L.S + TN * L.ld;
    L.sh = L.sc + padded(K);
    return L;
}
inline size_t lds_bytes(int K) {
    const int Kp = (K + KSTEP - 1) / KSTEP * KSTEP;
    return 2 * THREADS * sizeof(double) + ((size_t)TN * (Kp + 4) + 2 * (size_t)Kp) * sizeof(float);
}

// red[g * 16 + j] over the 64 row groups g, as a tree in a fixed order; every thread receives column j's sum
__device__ __forceinline__ double group_sum(double* red, double v, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int m = GROUPS / 2; m >= 1; m >>= 1) {
        if (tid < m * TN) red[tid] += red[tid + m * TN];
        __syncthreads();
    }
    const double r = red[tid & (TN - 1)];
    __syncthreads();
    return r;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
struct FwdTrunk {
    const float* in;          // [B,K]: the noise (layer 0) or the previous layer's Z; null = the trunk is not run
    const float* sc_prev;     // the previous layer's scale / shift [K]; null for layer 0
    const float* sh_prev;
    const float* w;           // [N,K]
    const float* bias;        // [N]
    const float* gamma;       // [N]   (trunk layers only, from here on)
    const float* beta;
    float* rmean;
    float* rvar;
    float* z;                 // [B,N]: the tape's Z (the head: y)
    float* scale;
    float* shift;
    double* mean;
    double* var;
    int N, K;
};
struct FwdArgs {
    FwdTrunk t[MAXT];
    long long B;
    float slope, eps, momentum;
    int training;
    int J;                    // the head: joints
    float* pose;              // the head: [B,J,3]
};

template <bool HEAD>
__global__ __launch_bounds__(THREADS) void gen_fwd_kernel(FwdArgs a) {
    extern __shared__ double lds_base[];
    const FwdTrunk T = a.t[blockIdx.y];
    const int n0 = blockIdx.x * TN;
    if (!T.in || n0 >= T.N) return;                             // (the whole workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int N = T.N, K = T.K, Kp = padded(K);
    const Lds L = carve_lds(lds_base, K);
    for (int i = tid; i < TN * Kp; i += THREADS) {
        const int j = i / Kp, k = i - j * Kp;
        L.S[j * L.ld + k] = (n0 + j < N && k < K) ? T.w[(size_t)(n0 + j) * K + k] : 0.f;
    }
    for (int k = tid; k < Kp; k += THREADS) {
        const bool on = T.sc_prev && k < K;
        L.sc[k] = on ? T.sc_prev[k] : 0.f;
        L.sh[k] = on ? T.sh_prev[k] : 0.f;
    }
    __syncthreads();
    const Operand op{T.in, T.sc_prev ? L.sc : nullptr, L.sh, a.slope};
    const int n = n0 + l15;
    const float bias = n < N ? T.bias[n] : 0.f;
    const long long tiles = (a.B + 15) / 16;
    for (long long rt = wv; rt < tiles; rt += WAVES) {
        float c[4];
        tile_product(op, L.S, L.ld, rt * 16, a.B, K, l15, l4, c);
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long b = rt * 16 + 4 * l4 + r;
                if (b < a.B) T.z[(size_t)b * N + n] = c[r] + bias;
            }
        }
    }
    __syncthreads();                                            // the workgroup's own Z is in memory for all its threads

    if (HEAD) {
        // joints n0 / 4 .. n0 / 4 + 3 of every row: four y columns each, all inside this tile
        for (long long i = tid; i < a.B * 4; i += THREADS) {
            const long long b = i >> 2;
            const int j = (n0 >> 2) + (int)(i & 3);
            if (j >= a.J) continue;
            const float* y = T.z + (size_t)b * N + 4 * j;
            const float a0 = y[0], a1 = y[1], a2 = y[2], th = y[3];
            const float nrm = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
            float o0 = a0 / nrm * th, o1 = a1 / nrm * th, o2 = a2 / nrm * th;
            if (j == 0) { o0 *= 6.28f; o1 *= 6.28f; o2 *= 6.28f; }
            float* o = a.pose + ((size_t)b * a.J + j) * 3;
            o[0] = o0; o[1] = o1; o[2] = o2;
        }
        return;
    }

    const int j = tid & (TN - 1), g = tid >> 4;
    const int nc = n0 + j;
    const bool live = nc < N;
    double mean, var;
    if (a.training) {
        double s = 0.0;
        if (live) {
            for (long long b = g; b < a.B; b += GROUPS) s += (double)T.z[(size_t)b * N + nc];
        }
        mean = group_sum(L.red0, s, tid) / (double)a.B;
        s = 0.0;
        if (live) {
            for (long long b = g; b < a.B; b += GROUPS) { const double d = (double)T.z[(size_t)b * N + nc] - mean; s += d * d; }
        }
        var = group_sum(L.red0, s, tid) / (double)a.B;
    } else {
        mean = live ? (double)T.rmean[nc] : 0.0;
        var = live ? (double)T.rvar[nc] : 1.0;
    }
    if (g != 0 || !live) return;
    const double sc = (double)T.gamma[nc] / sqrt(var + (double)a.eps);
    T.scale[nc] = (float)sc;
    T.shift[nc] = (float)((double)T.beta[nc] - mean * sc);
    T.mean[nc] = mean;
    T.var[nc] = var;
    if (a.training) {
        const double m = (double)a.momentum, unbiased = var * ((double)a.B / (double)(a.B - 1));
        T.rmean[nc] = (float)((1.0 - m) * (double)T.rmean[nc] + m * mean);
        T.rvar[nc] = (float)((1.0 - m) * (double)T.rvar[nc] + m * unbiased);
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
struct BwdTrunk {
    const float* dz_next;     // [B,Nn]: dZ of the layer above (the head: dy); null = `cot` is dH itself
    const float* w_next;      // [Nn,N]
    const float* cot;         // [B,N]
    const float* z;           // the layer's tape   (trunk layers only, from here on)
    const float* scale;
    const float* shift;
    const float* gamma;
    const double* mean;
    const double* var;
    float* out;               // [B,N]: dZ (the head: d_h); null = the trunk is skipped
    float* dgamma;            // [N] or null
    float* dbeta;
    int N, Nn;
};
struct BwdArgs {
    BwdTrunk t[MAXT];
    long long B;
    float slope, eps;
};

template <bool BN>
__global__ __launch_bounds__(THREADS) void gen_bwd_kernel(BwdArgs a) {
    extern __shared__ double lds_base[];
    const BwdTrunk T = a.t[blockIdx.y];
    const int n0 = blockIdx.x * TN;
    if (!T.out || n0 >= T.N) return;                            // (the whole workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int N = T.N, Nn = T.Nn;
    const Lds L = carve_lds(lds_base, T.dz_next ? Nn : 1);
    if (T.dz_next) {
        // the slab of W_next's columns n0 .. n0 + 15, transposed: S[j][k] = W_next[k, n0 + j]
        const int Kp = padded(Nn);
        for (int i = tid; i < TN * Kp; i += THREADS) {
            const int k = i / TN, j = i - k * TN;
            L.S[j * L.ld + k] = (n0 + j < N && k < Nn) ? T.w_next[(size_t)k * N + n0 + j] : 0.f;
        }
        __syncthreads();
        const Operand op{T.dz_next, nullptr, nullptr, 0.f};
        const int n = n0 + l15;
        float sc = 0.f, sh = 0.f;
        if (BN && n < N) { sc = T.scale[n]; sh = T.shift[n]; }
        const long long tiles = (a.B + 15) / 16;
        for (long long rt = wv; rt < tiles; rt += WAVES) {
            float c[4];
            tile_product(op, L.S, L.ld, rt * 16, a.B, Nn, l15, l4, c);
            if (n >= N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long b = rt * 16 + 4 * l4 + r;
                if (b >= a.B) continue;
                const size_t at = (size_t)b * N + n;
                float v = c[r];
                if (BN) v *= bn_pre(T.z[at], sc, sh) > 0.f ? 1.f : a.slope;
                T.out[at] = v;
            }
        }
        __syncthreads();                                        // dY of the workgroup's columns is in memory for all its threads
    }
    if (!BN) return;

    const int j = tid & (TN - 1), g = tid >> 4;
    const int nc = n0 + j;
    const bool live = nc < N;
    double mean = 0.0, invstd = 0.0;
    float sc = 0.f, sh = 0.f;
    if (live) { mean = T.mean[nc]; invstd = 1.0 / sqrt(T.var[nc] + (double)a.eps); sc = T.scale[nc]; sh = T.shift[nc]; }
    double s_beta = 0.0, s_gamma = 0.0;
    if (live) {
        for (long long b = g; b < a.B; b += GROUPS) {
            const size_t at = (size_t)b * N + nc;
            const float z = T.z[at];
            float dy;
            if (T.dz_next) dy = T.out[at];
            else { dy = T.cot[at] * (bn_pre(z, sc, sh) > 0.f ? 1.f : a.slope); T.out[at] = dy; }   // (read back below by this thread alone)
            s_beta += (double)dy;
            s_gamma += (double)dy * (((double)z - mean) * invstd);
        }
    }
    s_beta = group_sum(L.red0, s_beta, tid);
    s_gamma = group_sum(L.red1, s_gamma, tid);
    if (!live) return;
    const double k = (double)T.gamma[nc] * invstd / (double)a.B;
    for (long long b = g; b < a.B; b += GROUPS) {
        const size_t at = (size_t)b * N + nc;
        const double xh = ((double)T.z[at] - mean) * invstd;
        T.out[at] = (float)(k * ((double)a.B * (double)T.out[at] - s_beta - xh * s_gamma));
    }
    if (g == 0) {
        if (T.dgamma) T.dgamma[nc] = (float)s_gamma;
        if (T.dbeta) T.dbeta[nc] = (float)s_beta;
    }
}

// ---- weight gradients --------------------------------------------------------------------------------------------------------------------
constexpr int WT = 64, WTHREADS = 256, BK = 16, LDT = BK + 1, ROW_CHUNK = 64;   // disc_bwd_weight_kernel's tile and chunk fold
constexpr int MAXG = MAXT * MAXL;

struct WGroup {
    const float* dz;          // [B,N]
    const float* hin;         // [B,K]: the noise, or the Z of the layer below with its scale / shift
    const float* sc;
    const float* sh;
    float* dw;                // [N,K] or null
    float* db;                // [N] or null
    int N, K;
};
struct WArgs {
    WGroup g[MAXG];
    long long B;
    float slope;
};

__global__ __launch_bounds__(WTHREADS) void gen_wgrad_kernel(WArgs a) {
    __shared__ float sa[WT * LDT], sb[WT * LDT];
    const WGroup P = a.g[blockIdx.z];
    const int k0 = blockIdx.x * WT, n0 = blockIdx.y * WT;
    const bool bias_too = blockIdx.x == 0 && P.db;
    if (k0 >= P.K || n0 >= P.N || (!P.dw && !bias_too)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int j = tid & 63, rq = tid >> 6;
    float sc = 0.f, sh = 0.f;
    if (P.sc && k0 + j < P.K) { sc = P.sc[k0 + j]; sh = P.sh[k0 + j]; }
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
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long b = r0 + rq + 4 * c;
                sa[j * LDT + rq + 4 * c] = (n0 + j < P.N && b < c1) ? P.dz[(size_t)b * P.N + n0 + j] : 0.f;
                float v = 0.f;
                if (k0 + j < P.K && b < c1) {
                    v = P.hin[(size_t)b * P.K + k0 + j];
                    if (P.sc) v = lrelu(bn_pre(v, sc, sh), a.slope);
                }
                sb[j * LDT + rq + 4 * c] = v;
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
    if (P.dw) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 16 * w + 4 * l4 + r;
            if (n >= P.N) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = k0 + 16 * t + l15;
                if (k < P.K) P.dw[(size_t)n * P.K + k] = tot[t][r];
            }
        }
    }
    if (bias_too && tid < WT && n0 + tid < P.N) P.db[n0 + tid] = (float)tot_b;
}

// ---- the heads -------------------------------------------------------------------------------------------------------------------------
// dy [B,4J] of the bone-angle head from its tape y and the cotangent of pose, one thread per (row, joint), in double, rounded once
__global__ __launch_bounds__(256) void ba_head_dy_kernel(const float* __restrict__ y, const float* __restrict__ d_pose, long long B, int J,
                                                         float* __restrict__ dy) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * J) return;
    const int j = (int)(i % J);
    const float* yy = y + (size_t)i * 4;
    const float* gg = d_pose + (size_t)i * 3;
    const double a0 = yy[0], a1 = yy[1], a2 = yy[2], th = yy[3], g0 = gg[0], g1 = gg[1], g2 = gg[2];
    const double s = j == 0 ? (double)6.28f : 1.0;
    const double nrm = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    const double u0 = a0 / nrm, u1 = a1 / nrm, u2 = a2 / nrm;
    const double ug = u0 * g0 + u1 * g1 + u2 * g2;
    const double f = s * th / nrm;
    float* o = dy + (size_t)i * 4;
    o[0] = (float)(f * (g0 - u0 * ug));
    o[1] = (float)(f * (g1 - u1 * ug));
    o[2] = (float)(f * (g2 - u2 * ug));
    o[3] = (float)(s * ug);
}

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct RtArgs {
    const float* z_r;         // the R trunk's last Z [B,WR] with its scale / shift
    const float* sc_r;
    const float* sh_r;
    const float* z_t;         // the T trunk's last Z [B,WT]
    const float* sc_t;
    const float* sh_t;
    const float* w2;          // [3,WT]
    const float* b2;          // [3]
    const float* eps;         // [B,3]
    const float* x;           // [B,J,3]
    float* R;
    float* T;
    float* pose;
    long long B;
    int WR, WTw, J;
    float slope;
};

__global__ __launch_bounds__(256) void rt_head_kernel(RtArgs a) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;                                       // (whole waves)
    float t[3] = {0.f, 0.f, 0.f};
    const float* zt = a.z_t + (size_t)b * a.WTw;
    for (int k = lane; k < a.WTw; k += 64) {
        const float hv = lrelu(bn_pre(zt[k], a.sc_t[k], a.sh_t[k]), a.slope);
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = fmaf(hv, a.w2[(size_t)c * a.WTw + k], t[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = wave_sum_f32(t[c]) + a.b2[c];
    t[2] = t[2] * t[2];
    double r[7];
    const float* zr = a.z_r + (size_t)b * a.WR;
#pragma unroll
    for (int i = 0; i < 7; ++i) r[i] = (double)lrelu(bn_pre(zr[i], a.sc_r[i], a.sh_r[i]), a.slope);
    double ax[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ax[i] = r[i] + (r[3 + i] * r[3 + i]) * (double)a.eps[(size_t)b * 3 + i];
    const double nrm = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    double rv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) rv[i] = ax[i] / nrm * r[6];
    pgkin::Quat q;
    double rel[12];
    pgkin::rotvec_to_rows(rv, q, rel);
    float Rf[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rf[3 * i + c] = (float)rel[4 * i + c];
    if (lane < 9) a.R[(size_t)b * 9 + lane] = Rf[lane];
    if (lane < 3) a.T[(size_t)b * 3 + lane] = t[lane];
    const float* x = a.x + (size_t)b * a.J * 3;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    for (int e = lane; e < a.J * 3; e += 64) {
        const int jj = e / 3, c = e - 3 * jj;
        const float d0 = x[3 * jj] - x0, d1 = x[3 * jj + 1] - x1, d2 = x[3 * jj + 2] - x2;
        a.pose[(size_t)b * a.J * 3 + e] = fmaf(Rf[3 * c + 2], d2, fmaf(Rf[3 * c + 1], d1, Rf[3 * c] * d0)) + t[c];
    }
}

}  // namespace pggn

// ---- the host side -----------------------------------------------------------------------------------------------------------------------
namespace {

using namespace pggn;

// the backward's layer gradients and the head's dy: grow-only, one set per handle (calls on one handle are serialised by the caller)
struct GenState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_GEN;
    ~GenState() override { pg_release(dz); pg_release(dy); }
    DevBuf dz, dy;
};

int layers_of(const pg_gen_trunk& q) { return 1 + 2 * q.n_stages; }

const char* spec_fault(const pg_gen_spec* s) {
    if (!s) return "a null spec";
    if (s->n_trunks < 1 || s->n_trunks > MAXT) return "n_trunks outside [1, 4]";
    // (one rule for the slope across the loop's modules: posegen_gan.h reads its masks off the activations' sign, which a negative slope turns round)
    if (!(s->slope >= 0.f) || isinf(s->slope)) return "slope is negative or not finite";
    if (!(s->eps > 0.f) || isinf(s->eps)) return "eps is not positive and finite";
    if (!(s->momentum >= 0.f && s->momentum <= 1.f)) return "momentum outside [0, 1]";
    for (int t = 0; t < s->n_trunks; ++t) {
        const pg_gen_trunk& q = s->trunk[t];
        if (q.nz < 1 || q.nz > PG_GEN_MAX_DIM || q.width < 1 || q.width > PG_GEN_MAX_DIM) return "a trunk's nz or width outside [1, 512]";
        if (q.n_stages < 0 || q.n_stages > PG_GEN_MAX_STAGES) return "a trunk's n_stages outside [0, 4]";
    }
    return nullptr;
}

// where layer l of trunk t sits in a tape over B rows; t = n_trunks: the tape's end (z and mean are the two sizes)
struct Slot { int64_t z, scale, shift, mean, var; };
Slot slot_of(const pg_gen_spec& s, int64_t B, int t, int l) {
    int64_t f = 0, d = 0;
    for (int q = 0; q < t; ++q) { f += layers_of(s.trunk[q]) * (B + 2) * s.trunk[q].width; d += layers_of(s.trunk[q]) * 2 * (int64_t)s.trunk[q].width; }
    if (t >= s.n_trunks) return Slot{f, f, f, d, d};
    const int64_t W = s.trunk[t].width;
    f += l * (B + 2) * W; d += l * 2 * W;
    return Slot{f, f + B * W, f + B * W + W, d, d + W};
}

bool bad_f(const void* p) { return pg_misaligned(p, sizeof(float)); }

int check_common(pg_handle* h, const char* who, const pg_gen_spec* spec, int64_t B) {
    if (const char* f = spec_fault(spec)) return pg_fail(h, PG_EINVAL, "%s: %s", who, f);
    if (B < 1 || B > PG_GEN_MAX_ROWS) return pg_fail(h, PG_EINVAL, "%s: B = %lld is outside [1, %d]", who, (long long)B, PG_GEN_MAX_ROWS);
    return PG_OK;
}

int check_trunks(pg_handle* h, const char* who, const pg_gen_spec* spec, const pg_gen_params* params, const float* const* noise, const float* const* need,
                 int64_t B, const float* tape, const double* stats) {
    PG_TRY(check_common(h, who, spec, B));
    if (!params || !noise || !tape || !stats) return pg_fail(h, PG_EINVAL, "%s: params, noise, tape and stats are required", who);
    if (bad_f(tape) || pg_misaligned(stats, sizeof(double))) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    bool any = false;
    for (int t = 0; t < spec->n_trunks; ++t) {
        if (!need[t]) continue;
        any = true;
        if (!noise[t]) return pg_fail(h, PG_EINVAL, "%s: trunk %d has no noise", who, t);
        if (bad_f(noise[t]) || bad_f(need[t])) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
        for (int l = 0; l < layers_of(spec->trunk[t]); ++l) {
            const void* p[6] = {params->w[t][l], params->b[t][l], params->gamma[t][l], params->beta[t][l], params->running_mean[t][l], params->running_var[t][l]};
            for (const void* q : p)
                if (!q || bad_f(q)) return pg_fail(h, PG_EINVAL, "%s: trunk %d, layer %d: a parameter pointer is null or misaligned", who, t, l);
        }
    }
    if (!any) return pg_fail(h, PG_EINVAL, "%s: no trunk to run", who);
    return PG_OK;
}

int check_head(pg_handle* h, const char* who, const pg_gen_spec* spec, int trunk, int64_t B, int J) {
    PG_TRY(check_common(h, who, spec, B));
    if (trunk < 0 || trunk >= spec->n_trunks) return pg_fail(h, PG_EINVAL, "%s: trunk %d is outside [0, %d)", who, trunk, spec->n_trunks);
    if (J < 1 || J > PG_GEN_MAX_JOINTS) return pg_fail(h, PG_EINVAL, "%s: J = %d is outside [1, %d]", who, J, PG_GEN_MAX_JOINTS);
    return PG_OK;
}

unsigned ctiles(int n) { return (unsigned)((n + TN - 1) / TN); }
unsigned wtiles(int n) { return (unsigned)((n + WT - 1) / WT); }

}  // namespace

extern "C" int pg_gen_tape_size(const pg_gen_spec* spec, int64_t B, int64_t* n_floats, int64_t* n_doubles) {
    PG_TRY(check_common(nullptr, "pg_gen_tape_size", spec, B));
    if (!n_floats || !n_doubles) return pg_fail(nullptr, PG_EINVAL, "pg_gen_tape_size: no place for the result");
    const Slot end = slot_of(*spec, B, spec->n_trunks, 0);
    *n_floats = end.z;
    *n_doubles = end.mean;
    return PG_OK;
}

extern "C" int pg_gen_trunk_forward(pg_handle* h, void* stream, const pg_gen_spec* spec, const pg_gen_params* params, const float* const* noise,
                                    int64_t B, int32_t training, float* tape, double* stats) {
    const char* who = "pg_gen_trunk_forward";
    PG_TRY(check_trunks(h, who, spec, params, noise, noise, B, tape, stats));
    if (training && B < 2) return pg_fail(h, PG_EINVAL, "%s: training-mode statistics need B >= 2", who);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    const pg_gen_spec& s = *spec;
    PG_HIP(h, hipSetDevice(h->device));
    int max_layers = 0;
    for (int t = 0; t < s.n_trunks; ++t) if (noise[t] && layers_of(s.trunk[t]) > max_layers) max_layers = layers_of(s.trunk[t]);
    for (int l = 0; l < max_layers; ++l) {
        FwdArgs a{};
        a.B = B; a.slope = s.slope; a.eps = s.eps; a.momentum = s.momentum; a.training = training ? 1 : 0;
        int max_n = 0, max_k = 0;
        for (int t = 0; t < s.n_trunks; ++t) {
            if (!noise[t] || l >= layers_of(s.trunk[t])) continue;
            const Slot at = slot_of(s, B, t, l);
            FwdTrunk& T = a.t[t];
            T.N = s.trunk[t].width; T.K = l ? s.trunk[t].width : s.trunk[t].nz;
            if (l) {
                const Slot below = slot_of(s, B, t, l - 1);
                T.in = tape + below.z; T.sc_prev = tape + below.scale; T.sh_prev = tape + below.shift;
            } else {
                T.in = noise[t];
            }
            T.w = params->w[t][l]; T.bias = params->b[t][l]; T.gamma = params->gamma[t][l]; T.beta = params->beta[t][l];
            T.rmean = params->running_mean[t][l]; T.rvar = params->running_var[t][l];
            T.z = tape + at.z; T.scale = tape + at.scale; T.shift = tape + at.shift; T.mean = stats + at.mean; T.var = stats + at.var;
            max_n = T.N > max_n ? T.N : max_n;
            max_k = T.K > max_k ? T.K : max_k;
        }
        hipLaunchKernelGGL((gen_fwd_kernel<false>), dim3(ctiles(max_n), (unsigned)s.n_trunks), dim3(THREADS), lds_bytes(max_k),
                           static_cast<hipStream_t>(stream), a);
        PG_LAUNCH_CHECK(h, "generator layer kernel");
    }
    return PG_OK;
}

extern "C" int pg_gen_trunk_backward(pg_handle* h, void* stream, const pg_gen_spec* spec, const pg_gen_params* params, const float* const* noise,
                                     int64_t B, int32_t training, const float* tape, const double* stats, const float* const* d_out,
                                     const pg_gen_grads* grads) {
    const char* who = "pg_gen_trunk_backward";
    if (!training) return pg_fail(h, PG_EINVAL, "%s: the tape was written in eval mode; the backward of eval mode is not built", who);
    if (!d_out) return pg_fail(h, PG_EINVAL, "%s: d_out is required", who);
    PG_TRY(check_trunks(h, who, spec, params, noise, d_out, B, tape, stats));
    if (B < 2) return pg_fail(h, PG_EINVAL, "%s: training-mode statistics need B >= 2", who);
    const pg_gen_spec& s = *spec;
    if (grads)
        for (int t = 0; t < s.n_trunks; ++t)
            for (int l = 0; l < layers_of(s.trunk[t]); ++l)
                if (bad_f(grads->w[t][l]) || bad_f(grads->b[t][l]) || bad_f(grads->gamma[t][l]) || bad_f(grads->beta[t][l]))
                    return pg_fail(h, PG_EINVAL, "%s: trunk %d, layer %d: a gradient pointer is misaligned", who, t, l);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    GenState* st = nullptr;
    PG_TRY(pg_state(h, st));
    PG_HIP(h, hipSetDevice(h->device));
    // dZ of every layer of every trunk with a cotangent, laid out like the tape's Z
    int64_t dz_off[MAXT], dz_floats = 0;
    int max_layers = 0;
    for (int t = 0; t < s.n_trunks; ++t) {
        dz_off[t] = dz_floats;
        if (!d_out[t]) continue;
        dz_floats += (int64_t)layers_of(s.trunk[t]) * B * s.trunk[t].width;
        max_layers = layers_of(s.trunk[t]) > max_layers ? layers_of(s.trunk[t]) : max_layers;
    }
    PG_TRY(pg_grow(h, st->dz, (size_t)dz_floats * sizeof(float), "generator layer gradients"));
    float* dz = st->dz.as<float>();
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (int l = max_layers - 1; l >= 0; --l) {
        BwdArgs a{};
        a.B = B; a.slope = s.slope; a.eps = s.eps;
        int max_n = 0, max_k = 1;
        for (int t = 0; t < s.n_trunks; ++t) {
            const int L = layers_of(s.trunk[t]);
            if (!d_out[t] || l >= L) continue;
            const int W = s.trunk[t].width;
            const Slot at = slot_of(s, B, t, l);
            BwdTrunk& T = a.t[t];
            T.N = W; T.Nn = W;
            if (l == L - 1) {
                T.cot = d_out[t];
            } else {
                T.dz_next = dz + dz_off[t] + (int64_t)(l + 1) * B * W;
                T.w_next = params->w[t][l + 1];
                max_k = W > max_k ? W : max_k;
            }
            T.z = tape + at.z; T.scale = tape + at.scale; T.shift = tape + at.shift; T.gamma = params->gamma[t][l];
            T.mean = stats + at.mean; T.var = stats + at.var;
            T.out = dz + dz_off[t] + (int64_t)l * B * W;
            T.dgamma = grads ? grads->gamma[t][l] : nullptr;
            T.dbeta = grads ? grads->beta[t][l] : nullptr;
            max_n = W > max_n ? W : max_n;
        }
        hipLaunchKernelGGL((gen_bwd_kernel<true>), dim3(ctiles(max_n), (unsigned)s.n_trunks), dim3(THREADS), lds_bytes(max_k), hs, a);
        PG_LAUNCH_CHECK(h, "generator layer backward kernel");
    }
    if (!grads) return PG_OK;
    WArgs wa{};
    wa.B = B; wa.slope = s.slope;
    int n_groups = 0, max_n = 0, max_k = 0;
    for (int t = 0; t < s.n_trunks; ++t) {
        if (!d_out[t]) continue;
        for (int l = 0; l < layers_of(s.trunk[t]); ++l) {
            if (!grads->w[t][l] && !grads->b[t][l]) continue;
            WGroup& G = wa.g[n_groups++];
            const int W = s.trunk[t].width;
            G.N = W; G.K = l ? W : s.trunk[t].nz;
            G.dz = dz + dz_off[t] + (int64_t)l * B * W;
            if (l) {
                const Slot below = slot_of(s, B, t, l - 1);
                G.hin = tape + below.z; G.sc = tape + below.scale; G.sh = tape + below.shift;
            } else {
                G.hin = noise[t];
            }
            G.dw = grads->w[t][l]; G.db = grads->b[t][l];
            max_n = G.N > max_n ? G.N : max_n;
            max_k = G.K > max_k ? G.K : max_k;
        }
    }
    if (n_groups) {
        hipLaunchKernelGGL(gen_wgrad_kernel, dim3(wtiles(max_k), wtiles(max_n), (unsigned)n_groups), dim3(WTHREADS), 0, hs, wa);
        PG_LAUNCH_CHECK(h, "generator weight-gradient kernel");
    }
    return PG_OK;
}

extern "C" int pg_gen_ba_head_forward(pg_handle* h, void* stream, const pg_gen_spec* spec, int32_t trunk, const float* tape, int64_t B, int32_t J,
                                      const float* w2, const float* b2, float* y, float* pose) {
    const char* who = "pg_gen_ba_head_forward";
    PG_TRY(check_head(h, who, spec, trunk, B, J));
    if (!tape || !w2 || !b2 || !y || !pose) return pg_fail(h, PG_EINVAL, "%s: tape, w2, b2, y and pose are required", who);
    if (bad_f(tape) || bad_f(w2) || bad_f(b2) || bad_f(y) || bad_f(pose)) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    const pg_gen_spec& s = *spec;
    PG_HIP(h, hipSetDevice(h->device));
    const Slot last = slot_of(s, B, trunk, layers_of(s.trunk[trunk]) - 1);
    FwdArgs a{};
    a.B = B; a.slope = s.slope; a.J = J; a.pose = pose;
    FwdTrunk& T = a.t[0];
    T.in = tape + last.z; T.sc_prev = tape + last.scale; T.sh_prev = tape + last.shift;
    T.w = w2; T.bias = b2; T.z = y; T.N = 4 * J; T.K = s.trunk[trunk].width;
    hipLaunchKernelGGL((gen_fwd_kernel<true>), dim3(ctiles(T.N), 1u), dim3(THREADS), lds_bytes(T.K), static_cast<hipStream_t>(stream), a);
    PG_LAUNCH_CHECK(h, "generator bone-angle head kernel");
    return PG_OK;
}

extern "C" int pg_gen_ba_head_backward(pg_handle* h, void* stream, const pg_gen_spec* spec, int32_t trunk, const float* tape, int64_t B, int32_t J,
                                       const float* w2, const float* y, const float* d_pose, float* d_w2, float* d_b2, float* d_h) {
    const char* who = "pg_gen_ba_head_backward";
    PG_TRY(check_head(h, who, spec, trunk, B, J));
    if (!tape || !w2 || !y || !d_pose) return pg_fail(h, PG_EINVAL, "%s: tape, w2, y and d_pose are required", who);
    if (bad_f(tape) || bad_f(w2) || bad_f(y) || bad_f(d_pose) || bad_f(d_w2) || bad_f(d_b2) || bad_f(d_h))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    const pg_gen_spec& s = *spec;
    GenState* st = nullptr;
    PG_TRY(pg_state(h, st));
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(pg_grow(h, st->dy, (size_t)B * 4 * J * sizeof(float), "generator head gradient"));
    float* dy = st->dy.as<float>();
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int W = s.trunk[trunk].width;
    hipLaunchKernelGGL(ba_head_dy_kernel, dim3((unsigned)((B * J + 255) / 256)), dim3(256), 0, hs, y, d_pose, (long long)B, (int)J, dy);
    PG_LAUNCH_CHECK(h, "generator head dy kernel");
    if (d_h) {
        BwdArgs a{};
        a.B = B; a.slope = s.slope; a.eps = s.eps;
        BwdTrunk& T = a.t[0];
        T.dz_next = dy; T.w_next = w2; T.N = W; T.Nn = 4 * J; T.out = d_h;
        hipLaunchKernelGGL((gen_bwd_kernel<false>), dim3(ctiles(W), 1u), dim3(THREADS), lds_bytes(T.Nn), hs, a);
        PG_LAUNCH_CHECK(h, "generator head data-gradient kernel");
    }
    if (d_w2 || d_b2) {
        const Slot last = slot_of(s, B, trunk, layers_of(s.trunk[trunk]) - 1);
        WArgs wa{};
        wa.B = B; wa.slope = s.slope;
        wa.g[0] = WGroup{dy, tape + last.z, tape + last.scale, tape + last.shift, d_w2, d_b2, 4 * J, W};
        hipLaunchKernelGGL(gen_wgrad_kernel, dim3(wtiles(W), wtiles(4 * J), 1u), dim3(WTHREADS), 0, hs, wa);
        PG_LAUNCH_CHECK(h, "generator head weight-gradient kernel");
    }
    return PG_OK;
}

extern "C" int pg_gen_rt_head(pg_handle* h, void* stream, const pg_gen_spec* spec, int32_t trunk_r, int32_t trunk_t, const float* tape, int64_t B,
                              int32_t J, const float* w2_t, const float* b2_t, const float* eps, const float* x, float* R, float* T, float* pose_rt) {
    const char* who = "pg_gen_rt_head";
    PG_TRY(check_head(h, who, spec, trunk_r, B, J));
    PG_TRY(check_head(h, who, spec, trunk_t, B, J));
    if (spec->trunk[trunk_r].width < 7) return pg_fail(h, PG_EINVAL, "%s: the R trunk is narrower than 7", who);
    if (!tape || !w2_t || !b2_t || !eps || !x || !R || !T || !pose_rt)
        return pg_fail(h, PG_EINVAL, "%s: tape, w2_t, b2_t, eps, x, R, T and pose_rt are required", who);
    if (bad_f(tape) || bad_f(w2_t) || bad_f(b2_t) || bad_f(eps) || bad_f(x) || bad_f(R) || bad_f(T) || bad_f(pose_rt))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    const pg_gen_spec& s = *spec;
    PG_HIP(h, hipSetDevice(h->device));
    const Slot lr = slot_of(s, B, trunk_r, layers_of(s.trunk[trunk_r]) - 1), lt = slot_of(s, B, trunk_t, layers_of(s.trunk[trunk_t]) - 1);
    RtArgs a{tape + lr.z, tape + lr.scale, tape + lr.shift, tape + lt.z, tape + lt.scale, tape + lt.shift, w2_t, b2_t, eps, x, R, T, pose_rt,
             (long long)B, s.trunk[trunk_r].width, s.trunk[trunk_t].width, (int)J, s.slope};
    hipLaunchKernelGGL(rt_head_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PG_LAUNCH_CHECK(h, "generator rotation / translation head kernel");
    return PG_OK;
}
