// pg_smpl.hip -- the SMPL body on the device: smplx.lbs.lbs (smplx/smplx/lbs.py:152-248) with the joint regressors
// applied to its vertices (vertices2joints, :251-268), the mesh errors of run_gan.py:1630-1631 and the rotation-matrix form of the
// kinematic chain (get_smpl_l2ws_torch(axis_to_matrix=False), core/utils/skeleton_utils.py:379-463).
//   smpl_pre_kernel    : one wave per pose, lane j owns joint j.  Rodrigues as batch_rodrigues writes it (or the matrix as given), the
//                        rest joints from rest_joints and beta, the chain and the relative transforms A_j in float64; the pose's
//                        feature row f = [1, beta, (R_j - I), 0 ..] and A go to the workspace as float32, rounded once.
//   smpl_body_kernel   : a workgroup owns 32 poses and walks 64-vertex tiles.  Blend is a GEMM on v_mfma_f32_16x16x4_f32: A = the
//                        poses' feature rows (LDS), B = 192 columns of `blend` (each wave 48, read once per 32 poses), the result
//                        goes through LDS to the skinning lanes: T = sum_j skin[v,j] A_j is a second MFMA over the 24 joints (rows:
//                        4 poses x one row of T, columns: the wave's 16 vertices), so a lane receives a row of T for its (pose,
//                        vertex) and applies it.  The vertex goes to `verts` (if asked) and back into LDS, where the regressors
//                        meet it in a third MFMA (A = regress rows, B = 64 vertices x 96 (pose, xyz) columns).  One MFMA adds 4
//                        vertices in float32; everything above that is added in double, in tile order, per vertex chunk.
//   smpl_regress_sum   : the chunks' doubles added in chunk order, rounded to float32 once.
//   vertex_err_kernel, vertex_err_mean, kin_rot_kernel: one wave per pose, float64.
//   smpl_body_bwd_kernel, smpl_close_kernel: the transpose of the body (pg_smpl_backward), described where they stand.
// The vertex range is cut into 64-vertex tiles and min(tiles, 256) chunks (chunk c owns tiles c, c + chunks, ..): a function of V
// only.  A pose is a row of the first two MFMAs and three columns of the third, so its bytes do not depend on the batch around it.
// No atomics, no loop that depends on a value of the data.  The chain product and its transpose, the Rodrigues pair, the output writer
// of kin_rot_kernel and the check of a parents table are pg_kin.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_handle.h"
#include "pg_kin.h"

namespace pgsm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
using pgkin::NJ;
constexpr int POSE_ROWS = 207;               // 23 joints x 9
constexpr int MAX_NB = 16, MAX_K = 64;
constexpr int PT = 32;                       // poses per workgroup: two MFMA row tiles
constexpr int VT = 64;                       // vertices per tile: each wave 16 vertices = 48 columns = three MFMA column tiles
constexpr int KP_MAX = 224;                  // 1 + 16 + 207
constexpr int LDF = KP_MAX + 4;              // row stride of the feature tile: lanes (l & 15, l >> 4) fall on 64 different banks
constexpr int LDV = 3 * VT + 4;              // row stride of the vertex tile
constexpr int MAX_CHUNKS = 256;
constexpr size_t WS_TARGET = (size_t)48 << 20;

using pgkin::KinConst;
using pgkin::KinTree;
using pgkin::wave_all_sum;

// the rest joint of joint j and of its parent (zero for the root): linear in beta
__device__ __forceinline__ void rest_joint(const double* __restrict__ rest, const float* __restrict__ bp, int NB, int j, int par, double Jr[3],
                                           double Jp[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Jr[c] = rest[j * 3 + c];
        Jp[c] = par >= 0 ? rest[par * 3 + c] : 0.0;
    }
    for (int l = 0; l < NB; ++l) {
        const double b = (double)bp[l];
        const double* rl = rest + (size_t)(1 + l) * NJ * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Jr[c] += b * rl[j * 3 + c];
            if (par >= 0) Jp[c] += b * rl[par * 3 + c];
        }
    }
}

struct PreArgs {
    const float* betas;
    long long betas_stride;
    const float* pose;
    const double* rest;          // [1 + NB, 24, 3]
    float* feat;                 // [n, KP] or null
    float* A;                    // [n, 24, 12] or null
    float* joints;               // [n, 24, 3] or null
    long long n;
    int is_rotmat, NB, K, KP;
    KinTree tree;
};

__global__ __launch_bounds__(THREADS) void smpl_pre_kernel(PreArgs a) {
    __shared__ double srel[WAVES][NJ][12];
    __shared__ int spar[NJ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < NJ) spar[threadIdx.x] = a.tree.parent[threadIdx.x];
    long long pose = (long long)blockIdx.x * WAVES + w;
    const bool live = pose < a.n;                       // the whole wave
    if (!live) pose = a.n - 1;                          // computes a pose again and writes nothing
    const bool jl = lane < NJ;
    const int j = jl ? lane : 0;
    const int par = a.tree.parent[j];
    const float* bp = a.betas + pose * a.betas_stride;

    double Jr[3], Jp[3];
    rest_joint(a.rest, bp, a.NB, j, par, Jr, Jp);

    double G[12];                                       // the joint-to-parent transform [R | J - J_parent]
    if (a.is_rotmat) {
        pgkin::rotmat_to_rows(a.pose + ((size_t)pose * NJ + j) * 9, G);
    } else {
        pgkin::Rodrigues rg;                            // (what the map leaves for its transpose: not used here)
        pgkin::rodrigues_as_written(a.pose + ((size_t)pose * NJ + j) * 3, rg, G);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) G[4 * r + 3] = Jr[r] - Jp[r];

    // the feature row of the blend GEMM
    if (a.feat && live) {
        float* f = a.feat + (size_t)pose * a.KP;
        if (jl && j >= 1) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) f[1 + a.NB + (j - 1) * 9 + 3 * r + c] = (float)(G[4 * r + c] - (r == c ? 1.0 : 0.0));
        }
        if (lane == 0) f[0] = 1.f;
        if (lane >= 24 && lane < 24 + a.NB) f[1 + lane - 24] = bp[lane - 24];
        if (lane >= 48 && a.K + (lane - 48) < a.KP) f[a.K + (lane - 48)] = 0.f;
    }

    pgkin::chain_to_world(srel[w], spar, j, jl, a.tree.depth, G);

    if (live && jl) {
        if (a.joints) {
            float* o = a.joints + ((size_t)pose * NJ + j) * 3;
            o[0] = (float)G[3]; o[1] = (float)G[7]; o[2] = (float)G[11];
        }
        if (a.A) {
            // rel_transforms = transforms - pad(transforms @ [J; 0]) (lbs.py:396-399): [G_R | G_t - G_R J]
            float* o = a.A + ((size_t)pose * NJ + j) * 12;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)G[4 * r + c];
                o[4 * r + 3] = (float)(G[4 * r + 3] - (G[4 * r] * Jr[0] + G[4 * r + 1] * Jr[1] + G[4 * r + 2] * Jr[2]));
            }
        }
    }
}

struct BodyArgs {
    const float* blend;          // [K, 3V]
    const float* skin;           // [V, 24]
    const float* regress;        // [KR, V]
    const float* feat;           // [n, KP]
    const float* A;              // [n, 24, 12]
    float* verts;                // [n, V, 3] or null
    double* part;                // [chunks, n, KR, 3]
    long long n;
    int V, K, KP, KR, chunks, tiles;
};

__global__ __launch_bounds__(THREADS) void smpl_body_kernel(BodyArgs a) {
    __shared__ float sf[PT * LDF];
    __shared__ float sv[PT * LDV];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const long long pose0 = (long long)blockIdx.y * PT;
    const int V = a.V, KP = a.KP;
    const size_t ncol = (size_t)3 * V;

    // the feature rows: eight loads in flight per thread (a load per trip would pay the memory latency every trip)
    for (int i0 = tid; i0 < PT * KP; i0 += THREADS * 8) {
        float fv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * THREADS, row = i / KP;
            fv[u] = (i < PT * KP && pose0 + row < a.n) ? a.feat[(size_t)pose0 * KP + i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * THREADS, row = i / KP;
            if (i < PT * KP) sf[row * LDF + (i - row * KP)] = fv[u];
        }
    }
    __syncthreads();

    const int MT = (a.KR + 15) >> 4, P = 6 * MT;         // regressor row tiles; (row tile, column tile) products of the workgroup
    double racc[6][4];
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) racc[q][r] = 0.0;

    for (int tile = blockIdx.x; tile < a.tiles; tile += a.chunks) {
        const int v0 = tile * VT;
        // ---- blend: v_posed[32 poses, the wave's 48 columns] ----
        f32x4 acc[2][3];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const size_t c0 = (size_t)3 * v0 + w * 48 + l15;
        // eight k steps at a time: their 24 B fragments are loaded together, then the 48 MFMAs run (rows past K, and features past
        // KP, are zero: the steps a short last group adds change nothing)
        for (int k0 = 0; k0 < KP; k0 += 32) {
            float b[8][3];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int kk = k0 + 4 * s + l4;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const size_t col = c0 + t * 16;
                    b[s][t] = (kk < a.K && col < ncol) ? a.blend[(size_t)kk * ncol + col] : 0.f;
                }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int kk = k0 + 4 * s + l4;
                const float a0 = kk < KP ? sf[l15 * LDF + kk] : 0.f, a1 = kk < KP ? sf[(16 + l15) * LDF + kk] : 0.f;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[s][t], acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[s][t], acc[1][t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) sv[(m * 16 + l4 * 4 + r) * LDV + w * 48 + t * 16 + l15] = acc[m][t][r];
        __syncthreads();

        // ---- skinning: T = sum_j skin[v,j] A_j as an MFMA over the 24 joints.  Rows: 4 poses x the 4 entries of row c of T;
        //      columns: the wave's own 16 vertices.  A lane receives row c of T for its (pose, vertex), three times: T [v; 1] ----
        const int v = v0 + w * 16 + l15;
        const bool vlive = v < V;
        float sk[NJ / 4];
#pragma unroll
        for (int ks = 0; ks < NJ / 4; ++ks) sk[ks] = vlive ? a.skin[(size_t)v * NJ + 4 * ks + l4] : 0.f;
        for (int pb = 0; pb < PT / 4; ++pb) {
            const long long apose = pose0 + 4 * pb + (l15 >> 2);         // the pose of the lane's A row; its entry: l15 & 3
            const bool alive = apose < a.n;
            const float* Ar = a.A + (size_t)(alive ? apose : 0) * (NJ * 12) + 12 * l4 + (l15 & 3);     // + 48 ks + 4 c
            const int row = 4 * pb + l4;                                 // the pose of the lane's results
            const long long pose = pose0 + row;
            float* pv = sv + row * LDV + 3 * (w * 16 + l15);
            const float x = pv[0], y = pv[1], z = pv[2];
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 T = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < NJ / 4; ++ks)
                    T = __builtin_amdgcn_mfma_f32_16x16x4f32(alive ? Ar[48 * ks + 4 * c] : 0.f, sk[ks], T, 0, 0, 0);
                o[c] = vlive ? fmaf(T[0], x, fmaf(T[1], y, fmaf(T[2], z, T[3]))) : 0.f;
            }
            if (a.verts && vlive && pose < a.n) {
                float* ov = a.verts + ((size_t)pose * V + v) * 3;
                ov[0] = o[0]; ov[1] = o[1]; ov[2] = o[2];
            }
            pv[0] = o[0]; pv[1] = o[1]; pv[2] = o[2];
        }

        // ---- regression: regress[KR, 64 vertices] x verts[64 vertices, 32 poses x 3] ----
        if (a.KR > 0) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int p = w + WAVES * q;
                if (p < P) {                             // the whole wave
                    const int mt = p / 6, nt = p - mt * 6;
                    const int krow = mt * 16 + l15, jj = nt * 16 + l15;
                    const int jb = jj / 3, jc = jj - jb * 3;
                    const bool klive = krow < a.KR;
                    const float* rrow = a.regress + (size_t)(klive ? krow : 0) * V;
                    float ra[VT / 4];                    // the product's 16 regressor fragments, loaded together
#pragma unroll
                    for (int s = 0; s < VT / 4; ++s) ra[s] = (klive && v0 + 4 * s + l4 < V) ? rrow[v0 + 4 * s + l4] : 0.f;
#pragma unroll
                    for (int s4 = 0; s4 < VT / 4; ++s4) {
                        const int kk = 4 * s4 + l4;
                        const float rb = sv[jb * LDV + 3 * kk + jc];
                        const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[s4], rb, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) racc[q][r] += (double)d[r];
                    }
                }
            }
        }
        __syncthreads();
    }

    if (a.KR > 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int p = w + WAVES * q;
            if (p < P) {
                const int mt = p / 6, nt = p - mt * 6;
                const int jj = nt * 16 + l15;
                const int jb = jj / 3, jc = jj - jb * 3;
                const long long pose = pose0 + jb;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = mt * 16 + l4 * 4 + r;
                    if (k < a.KR && pose < a.n) a.part[(((size_t)blockIdx.x * a.n + pose) * a.KR + k) * 3 + jc] = racc[q][r];
                }
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void smpl_regress_sum(const double* __restrict__ part, long long per_chunk, int chunks,
                                                            float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= per_chunk) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * per_chunk + i];
    out[i] = (float)s;
}

// per_pose[b] = mean_v |a_v - b_v| (run_gan.py:1630-1631): lane l adds vertices l, l + 64, .. in that order, then the butterfly
__global__ __launch_bounds__(THREADS) void vertex_err_kernel(const float* __restrict__ a, const float* __restrict__ b, long long B, int V,
                                                             double* __restrict__ per_pose) {
    const int lane = threadIdx.x & 63;
    const long long pose = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (pose >= B) return;                               // the whole wave
    const float* pa = a + (size_t)pose * V * 3;
    const float* pb = b + (size_t)pose * V * 3;
    double s = 0.0;
    for (int v = lane; v < V; v += 64) {
        const double dx = (double)pa[3 * (size_t)v] - (double)pb[3 * (size_t)v], dy = (double)pa[3 * (size_t)v + 1] - (double)pb[3 * (size_t)v + 1],
                     dz = (double)pa[3 * (size_t)v + 2] - (double)pb[3 * (size_t)v + 2];
        s += sqrt(dx * dx + dy * dy + dz * dz);
    }
    s = wave_all_sum(s);
    if (lane == 0) per_pose[pose] = s / (double)V;
}

// summary = B, the mean of per_pose: thread t adds poses t, t + 256, .. in that order, the four waves' sums are added in wave order
__global__ __launch_bounds__(THREADS) void vertex_err_mean(const double* __restrict__ per_pose, long long B, double* __restrict__ summary) {
    __shared__ double sw[WAVES];
    double s = 0.0;
    for (long long i = threadIdx.x; i < B; i += THREADS) s += per_pose[i];
    s = wave_all_sum(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        summary[0] = (double)B;
        summary[1] = (((sw[0] + sw[1]) + sw[2]) + sw[3]) / (double)B;
    }
}

// get_smpl_l2ws_torch(axis_to_matrix=False): l2w_j = l2w_parent [R_j | rest_j - rest_parent], float64 on the float32 matrices
__global__ __launch_bounds__(THREADS) void kin_rot_kernel(const KinConst kc, const float* __restrict__ rot, long long n, float* __restrict__ kps,
                                                          float* __restrict__ skts, double* __restrict__ l2ws) {
    __shared__ double srel[WAVES][NJ][12];
    __shared__ int spar[NJ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < NJ) spar[threadIdx.x] = kc.tree.parent[threadIdx.x];
    long long pose = (long long)blockIdx.x * WAVES + w;
    const bool live = pose < n;
    if (!live) pose = n - 1;
    const bool jl = lane < NJ;
    const int j = jl ? lane : 0;
    double G[12];
    pgkin::rotmat_to_rows(rot + ((size_t)pose * NJ + j) * 9, G);
#pragma unroll
    for (int r = 0; r < 3; ++r) G[4 * r + 3] = kc.offs[3 * j + r];
    pgkin::chain_to_world(srel[w], spar, j, jl, kc.tree.depth, G);
    if (!live || !jl) return;
    pgkin::write_pose_outputs(G, (size_t)pose * NJ + j, kps, l2ws, skts);
}

// ---- the transpose of the body -------------------------------------------------------------------------------------
//   smpl_body_bwd_kernel : the forward's tiling.  Per 64-vertex tile: v_posed again (the forward's blend GEMM, the same bytes); the
//                          vertex cotangent dv = d_verts + regress^T d_regressed (an MFMA over the regressor rows); T again and
//                          d v_posed = T_R^T dv; dA[pose, entry; joint] += skin (dv (x) [v_posed; 1]) (an MFMA over the tile's
//                          vertices, rows = 16 poses x one entry of the 3 x 4); d feat[pose, k] += blend[k, :] d v_posed (an MFMA
//                          over the tile's 192 columns, B from blend_t, or from blend strided).  One tile is added in float32
//                          inside the MFMAs; tiles are added in double, in tile order, per vertex chunk.
//   smpl_close_kernel    : one wave per pose, lane = joint, float64.  The chunks' partials in chunk order, d_joints into the
//                          translation cotangent of G, A = [G_R | G_t - G_R J] undone, the chain walked back level by level in LDS
//                          (chain_backward, pg_kin.h), dJ into d_betas through rest_joints, the d feat rows for beta and
//                          R_j - I, Rodrigues transposed or the nine entries; rounded to float32 once.
constexpr int BWD_MAX_CHUNKS = 64;           // a pose and chunk leave BWD_PART doubles, ten times the forward's partials
constexpr int BWD_PART = NJ * 12 + KP_MAX;   // dA [24][12], then d feat [224]
constexpr size_t BWD_WS_TARGET = (size_t)96 << 20;
constexpr int LDR = MAX_K + 4;               // row stride of the d_regressed tile: lanes (l & 15, l >> 4) on 64 different banks
constexpr int FCT = (KP_MAX / 16 + WAVES - 1) / WAVES;   // d feat column tiles of a wave

struct BwdArgs {
    const float* blend;          // [K, 3V]
    const float* blend_t;        // [3V, K] or null
    const float* skin;           // [V, 24]
    const float* regress;        // [KR, V]
    const float* feat;           // [n, KP]
    const float* A;              // [n, 24, 12]
    const float* d_verts;        // [n, V, 3] or null
    const float* d_reg;          // [n, KR, 3] or null (KR = 0)
    double* part;                // [chunks, n, BWD_PART]
    long long n;
    int V, K, KP, KR, chunks, tiles;
};

__global__ __launch_bounds__(THREADS) void smpl_body_bwd_kernel(BwdArgs a) {
    __shared__ float sf[PT * LDF];
    __shared__ float sv[PT * LDV];               // v_posed
    __shared__ float sd[PT * LDV];               // dv
    __shared__ float sp[PT * LDV];               // d v_posed
    __shared__ float sr[3 * PT * LDR];           // d_regressed: row (pose, xyz), column = regressor row
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const long long pose0 = (long long)blockIdx.y * PT;
    const int V = a.V, KP = a.KP, KR = a.KR;
    const size_t ncol = (size_t)3 * V;

    for (int i0 = tid; i0 < PT * KP; i0 += THREADS * 8) {
        float fv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * THREADS, row = i / KP;
            fv[u] = (i < PT * KP && pose0 + row < a.n) ? a.feat[(size_t)pose0 * KP + i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * THREADS, row = i / KP;
            if (i < PT * KP) sf[row * LDF + (i - row * KP)] = fv[u];
        }
    }
    if (KR > 0) {
        for (int i = tid; i < 3 * PT * MAX_K; i += THREADS) {
            const int jj = i / MAX_K, k = i - jj * MAX_K, p = jj / 3, c = jj - p * 3;
            sr[jj * LDR + k] = (k < KR && pose0 + p < a.n) ? a.d_reg[((size_t)(pose0 + p) * KR + k) * 3 + c] : 0.f;
        }
    }
    __syncthreads();

    double accA[6][2][4], accF[FCT][2][4];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) accA[i][t][r] = 0.0;
#pragma unroll
    for (int i = 0; i < FCT; ++i)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) accF[i][m][r] = 0.0;

    for (int tile = blockIdx.x; tile < a.tiles; tile += a.chunks) {
        const int v0 = tile * VT;
        // ---- (a) v_posed[32 poses, the wave's 48 columns]: the forward's blend GEMM, step for step ----
        {
            f32x4 acc[2][3];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            const size_t c0 = (size_t)3 * v0 + w * 48 + l15;
            for (int k0 = 0; k0 < KP; k0 += 32) {
                float b[8][3];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int kk = k0 + 4 * s + l4;
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const size_t col = c0 + t * 16;
                        b[s][t] = (kk < a.K && col < ncol) ? a.blend[(size_t)kk * ncol + col] : 0.f;
                    }
                }
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int kk = k0 + 4 * s + l4;
                    const float a0 = kk < KP ? sf[l15 * LDF + kk] : 0.f, a1 = kk < KP ? sf[(16 + l15) * LDF + kk] : 0.f;
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[s][t], acc[0][t], 0, 0, 0);
                        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[s][t], acc[1][t], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sv[(m * 16 + l4 * 4 + r) * LDV + w * 48 + t * 16 + l15] = acc[m][t][r];
        }
        // the tile of d_verts: a pose's 192 values are contiguous (zero past the last vertex, past the last pose, or without d_verts)
        for (int i0 = tid; i0 < PT * 3 * VT; i0 += THREADS * 8) {
            float dvv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * THREADS, p = i / (3 * VT);
                const size_t col = (size_t)3 * v0 + (i - p * 3 * VT);
                dvv[u] = (a.d_verts && pose0 + p < a.n && col < ncol) ? a.d_verts[(size_t)(pose0 + p) * ncol + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * THREADS, p = i / (3 * VT);
                sd[p * LDV + (i - p * 3 * VT)] = dvv[u];
            }
        }
        __syncthreads();

        const int v = v0 + w * 16 + l15;                 // the wave's own 16 vertices, as in the forward
        const bool vlive = v < V;
        // ---- (b) dv += regress^T d_regressed: rows (pose, xyz), columns the wave's vertices, k over the regressor rows ----
        if (KR > 0) {
            float rb[MAX_K / 4];
#pragma unroll
            for (int s = 0; s < MAX_K / 4; ++s) rb[s] = (4 * s + l4 < KR && vlive) ? a.regress[(size_t)(4 * s + l4) * V + v] : 0.f;
#pragma unroll
            for (int nt = 0; nt < 6; ++nt) {
                f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < MAX_K / 4; ++s)
                    if (4 * s < KR) d = __builtin_amdgcn_mfma_f32_16x16x4f32(sr[(nt * 16 + l15) * LDR + 4 * s + l4], rb[s], d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jj = nt * 16 + l4 * 4 + r, jb = jj / 3, jc = jj - jb * 3;
                    sd[jb * LDV + 3 * (w * 16 + l15) + jc] += d[r];
                }
            }
            __syncthreads();
        }

        // ---- (c) T = sum_j skin[v,j] A_j as in the forward; d v_posed = T_R^T dv ----
        {
            float sk[NJ / 4];
#pragma unroll
            for (int ks = 0; ks < NJ / 4; ++ks) sk[ks] = vlive ? a.skin[(size_t)v * NJ + 4 * ks + l4] : 0.f;
            for (int pb = 0; pb < PT / 4; ++pb) {
                const long long apose = pose0 + 4 * pb + (l15 >> 2);
                const bool alive = apose < a.n;
                const float* Ar = a.A + (size_t)(alive ? apose : 0) * (NJ * 12) + 12 * l4 + (l15 & 3);
                const int at = (4 * pb + l4) * LDV + 3 * (w * 16 + l15);
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 T = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < NJ / 4; ++ks)
                        T = __builtin_amdgcn_mfma_f32_16x16x4f32(alive ? Ar[48 * ks + 4 * c] : 0.f, sk[ks], T, 0, 0, 0);
                    const float dvc = sd[at + c];
                    g0 = fmaf(T[0], dvc, g0); g1 = fmaf(T[1], dvc, g1); g2 = fmaf(T[2], dvc, g2);
                }
                sp[at] = vlive ? g0 : 0.f; sp[at + 1] = vlive ? g1 : 0.f; sp[at + 2] = vlive ? g2 : 0.f;
            }
        }
        __syncthreads();

        // ---- (d) dA: row tile = (entry of the 3 x 4, 16 poses), the wave's six; columns = joints; k over the tile's vertices ----
        {
            float skb[VT / 4][2];
#pragma unroll
            for (int s = 0; s < VT / 4; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int vv = v0 + 4 * s + l4, j = t * 16 + l15;
                    skb[s][t] = (vv < V && j < NJ) ? a.skin[(size_t)vv * NJ + j] : 0.f;
                }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int rt = w * 6 + i, e = rt >> 1, er = e >> 2, ec = e & 3;
                const int base = ((rt & 1) * 16 + l15) * LDV + 3 * l4;
                f32x4 d0 = f32x4{0.f, 0.f, 0.f, 0.f}, d1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < VT / 4; ++s) {
                    const float x = sd[base + 12 * s + er] * (ec < 3 ? sv[base + 12 * s + ec] : 1.f);
                    d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x, skb[s][0], d0, 0, 0, 0);
                    d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x, skb[s][1], d1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) { accA[i][0][r] += (double)d0[r]; accA[i][1][r] += (double)d1[r]; }
            }
        }

        // ---- (e) d feat: rows = poses, columns = blend rows (the wave's tiles w, w + 4, ..), k over the tile's 192 columns ----
        {
            f32x4 acc[FCT][2];
#pragma unroll
            for (int i = 0; i < FCT; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            for (int s0 = 0; s0 < 3 * VT / 4; s0 += 8) {
                float b[8][FCT];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const size_t col = (size_t)3 * v0 + 4 * (s0 + s) + l4;
#pragma unroll
                    for (int i = 0; i < FCT; ++i) {
                        const int k = (w + WAVES * i) * 16 + l15;
                        b[s][i] = (k < a.K && col < ncol) ? (a.blend_t ? a.blend_t[col * a.K + k] : a.blend[(size_t)k * ncol + col]) : 0.f;
                    }
                }
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const float a0 = sp[l15 * LDV + 4 * (s0 + s) + l4], a1 = sp[(16 + l15) * LDV + 4 * (s0 + s) + l4];
#pragma unroll
                    for (int i = 0; i < FCT; ++i)
                        if ((w + WAVES * i) * 16 < KP_MAX) {
                            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[s][i], acc[i][0], 0, 0, 0);
                            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[s][i], acc[i][1], 0, 0, 0);
                        }
                }
            }
#pragma unroll
            for (int i = 0; i < FCT; ++i)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) accF[i][m][r] += (double)acc[i][m][r];
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int rt = w * 6 + i, e = rt >> 1;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * 16 + l15;
                const long long pose = pose0 + (rt & 1) * 16 + l4 * 4 + r;
                if (j < NJ && pose < a.n) a.part[((size_t)blockIdx.x * a.n + pose) * BWD_PART + j * 12 + e] = accA[i][t][r];
            }
    }
#pragma unroll
    for (int i = 0; i < FCT; ++i) {
        const int k = (w + WAVES * i) * 16 + l15;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long pose = pose0 + m * 16 + l4 * 4 + r;
                if (k < KP_MAX && pose < a.n) a.part[((size_t)blockIdx.x * a.n + pose) * BWD_PART + NJ * 12 + k] = accF[i][m][r];
            }
    }
}

struct CloseArgs {
    const float* betas;
    long long betas_stride;
    const float* pose;
    const double* rest;          // [1 + NB, 24, 3]
    const double* part;          // [chunks, n, BWD_PART] (chunks = 0: no vertex-tile kernel ran)
    const float* d_joints;       // [n, 24, 3] or null
    float* d_betas;              // [n, NB] or null
    float* d_pose;               // [n, 24, 3] or [n, 24, 3, 3], or null
    long long n;
    int is_rotmat, NB, chunks;
    KinTree tree;
};

__global__ __launch_bounds__(THREADS) void smpl_close_kernel(CloseArgs a) {
    __shared__ double rel[WAVES][NJ][12], l2w[WAVES][NJ][12], Gc[WAVES][NJ][12];
    __shared__ double sJ[WAVES][NJ][3], sfe[WAVES][KP_MAX];
    __shared__ int spar[NJ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < NJ) spar[threadIdx.x] = a.tree.parent[threadIdx.x];
    long long pose = (long long)blockIdx.x * WAVES + w;
    const bool live = pose < a.n;                       // the whole wave
    if (!live) pose = a.n - 1;                          // walks the last pose again and writes nothing
    const bool jl = lane < NJ;
    const int j = jl ? lane : 0;
    const int par = a.tree.parent[j], lev = a.tree.level[j];
    const float* bp = a.betas + pose * a.betas_stride;

    // 1. the forward in double, as smpl_pre_kernel: rest joints, R, the relative transform [R | J - J_parent], the chain
    double Jr[3], Jp[3];
    rest_joint(a.rest, bp, a.NB, j, par, Jr, Jp);
    double M[12];
    pgkin::Rodrigues rg{};
    if (a.is_rotmat) {
        pgkin::rotmat_to_rows(a.pose + ((size_t)pose * NJ + j) * 9, M);
    } else {
        pgkin::rodrigues_as_written(a.pose + ((size_t)pose * NJ + j) * 3, rg, M);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) M[4 * r + 3] = Jr[r] - Jp[r];
    pgkin::chain_forward(rel[w], l2w[w], M, j, jl, par, lev, a.tree.depth);

    // 2. the chunks' partials in chunk order: dA of the lane's joint, d feat four columns a lane
    double dA[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) dA[e] = 0.0;
    for (int k = lane; k < KP_MAX; k += 64) {
        double s = 0.0;
        for (int c = 0; c < a.chunks; ++c) s += a.part[((size_t)c * a.n + pose) * BWD_PART + NJ * 12 + k];
        sfe[w][k] = s;
    }
    if (jl) {
        for (int c = 0; c < a.chunks; ++c) {
            const double* p = a.part + ((size_t)c * a.n + pose) * BWD_PART + j * 12;
#pragma unroll
            for (int e = 0; e < 12; ++e) dA[e] += p[e];
        }
    }

    // 3. A = [G_R | G_t - G_R J] undone: dG_R = dA_R - dA_t (x) J, dG_t = dA_t + d_joints, dJ = -G_R^T dA_t
    double dJ[3] = {0.0, 0.0, 0.0};
    if (jl) {
        const double* G = l2w[w][j];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double t = dA[4 * r + 3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Gc[w][j][4 * r + c] = dA[4 * r + c] - t * Jr[c];
                dJ[c] -= G[4 * r + c] * t;
            }
            Gc[w][j][4 * r + 3] = t + (a.d_joints ? (double)a.d_joints[((size_t)pose * NJ + j) * 3 + r] : 0.0);
        }
    }
    __syncthreads();
    // 4. the chain backwards, children before parents
    pgkin::chain_backward(Gc[w], rel[w], spar, j, jl, lev, a.tree.depth);
    // 5. the cotangent of the relative transform: G_parent_R^T dG (the root's parent is the identity); its column 3 is d(J - J_parent)
    double D[12];
    pgkin::parent_transpose<4>(l2w[w], par, Gc[w][j], D);
    __syncthreads();                                    // every lane has read l2w and Gc: rel's rows now carry d(J - J_parent)
    if (jl) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { rel[w][j][c] = D[4 * c + 3]; dJ[c] += D[4 * c + 3]; }
    }
    __syncthreads();
    if (jl) {
        for (int c = j + 1; c < NJ; ++c) {
            if (spar[c] != j) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) dJ[k] -= rel[w][c][k];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) sJ[w][j][c] = dJ[c];
    }
    __syncthreads();
    if (!live) return;

    // 6. d_betas: the d feat row of beta_l plus dJ through rest_joints[1 + l]
    if (a.d_betas && lane < a.NB) {
        double s = sfe[w][1 + lane];
        const double* rl = a.rest + (size_t)(1 + lane) * NJ * 3;
        for (int q = 0; q < NJ * 3; ++q) s += rl[q] * sJ[w][q / 3][q - (q / 3) * 3];
        a.d_betas[(size_t)pose * a.NB + lane] = (float)s;
    }
    if (!a.d_pose || !jl) return;
    // 7. dR: the chain's plus, for joints 1.., the d feat rows of R_j - I; the nine entries, or through batch_rodrigues as written
    double dR[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) dR[3 * r + c] = D[4 * r + c] + (j >= 1 ? sfe[w][1 + a.NB + (j - 1) * 9 + 3 * r + c] : 0.0);
    if (a.is_rotmat) {
        float* dst = a.d_pose + ((size_t)pose * NJ + j) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) dst[e] = (float)dR[e];
        return;
    }
    double o[3];
    pgkin::rodrigues_as_written_bwd(rg, dR, o);
    float* dst = a.d_pose + ((size_t)pose * NJ + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (float)o[c];
}

}  // namespace pgsm

// ---- the host side --------------------------------------------------------------------------------------------------------------------
namespace {

struct SmplState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_SMPL;
    ~SmplState() override { pg_release(ws); }
    DevBuf ws;
};

// what pg_smpl_forward and pg_smpl_backward share of a call, once it is valid
struct BodyPlan {
    int rows, KP, tiles;         // blend rows 1 + NB + 207, rounded up to a multiple of 4; 64-vertex tiles
    pgkin::KinTree tree;
    float* feat = nullptr;       // the slice's workspace
    float* A = nullptr;
    double* part = nullptr;
};

// The checks of a body call.  `missing`: what the entry point found it was not given or asked for (null: nothing); `reg`: how it
// names its regressor-side array when it has one (null: none).
int body_plan(pg_handle* h, const char* who, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride, const float* pose,
              const float* regress, int K, const char* missing, const char* reg, BodyPlan& p) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!m || !betas || !pose) return pg_fail(h, PG_EINVAL, "%s: model, betas and pose are required", who);
    if (missing) return pg_fail(h, PG_EINVAL, "%s: %s", who, missing);
    if (B < 1) return pg_fail(h, PG_EINVAL, "%s: B = %lld", who, (long long)B);
    if (m->NB < 1 || m->NB > pgsm::MAX_NB) return pg_fail(h, PG_EINVAL, "%s: NB = %d is outside [1, %d]", who, m->NB, pgsm::MAX_NB);
    p.rows = 1 + m->NB + pgsm::POSE_ROWS;
    if (m->V < 1 || (long long)p.rows * 3 * (long long)m->V >= (1ll << 31))
        return pg_fail(h, PG_EINVAL, "%s: V = %d (at least 1, and %d blend rows of 3 V below 2^31 elements)", who, m->V, p.rows);
    if (!m->blend || !m->skin || !m->rest_joints) return pg_fail(h, PG_EINVAL, "%s: the model has a NULL array", who);
    if (K < 0 || K > pgsm::MAX_K) return pg_fail(h, PG_EINVAL, "%s: K = %d is outside [0, %d]", who, K, pgsm::MAX_K);
    if (K > 0 && !regress) return pg_fail(h, PG_EINVAL, "%s: K = %d without regress", who, K);
    if (reg && K == 0) return pg_fail(h, PG_EINVAL, "%s: %s with K = 0", who, reg);
    if (betas_stride != 0 && betas_stride != m->NB)
        return pg_fail(h, PG_EINVAL, "%s: betas_stride = %lld (NB = %d, or 0 for one row)", who, (long long)betas_stride, m->NB);
    if (m->parents[0] != -1 || !pgkin::pg_kin_tree(m->parents, p.tree))
        return pg_fail(h, PG_EINVAL, "%s: parents[0] must be -1 and every joint must come after its parent", who);
    p.KP = (p.rows + 3) & ~3;
    p.tiles = (m->V + pgsm::VT - 1) / pgsm::VT;
    return PG_OK;
}

// the poses of one slice: what keeps a workspace of per_pose bytes a pose at `target`, in whole pose tiles, at least one, 4096 at most
long long slice_poses(size_t per_pose, size_t target) {
    const long long S = (long long)(target / per_pose) / pgsm::PT * pgsm::PT;
    return S < pgsm::PT ? pgsm::PT : S > 4096 ? 4096 : S;
}

// the workspace of a slice of S poses: the chunks' partials (part_doubles of them; none: null), the feature rows and A
int carve_body(pg_handle* h, BodyPlan& p, size_t part_doubles, long long S) {
    SmplState* s = nullptr;
    PG_TRY(pg_state(h, s));
    auto carve = [&](Carver& c) {
        p.part = c.take<double>(part_doubles, part_doubles > 0);
        p.feat = c.take<float>((size_t)S * p.KP);
        p.A = c.take<float>((size_t)S * pgsm::NJ * 12);
    };
    Carver count, real;
    carve(count);
    PG_TRY(pg_grow(h, s->ws, count.off, "body model workspace"));
    real.base = s->ws.p;
    carve(real);
    return PG_OK;
}

int launch_pre(pg_handle* h, hipStream_t st, const BodyPlan& p, const pg_body_model* m, const float* betas, int64_t betas_stride,
               const float* pose, int pose_is_rotmat, float* joints, long long n) {
    pgsm::PreArgs pa{};
    pa.betas = betas; pa.betas_stride = betas_stride; pa.pose = pose; pa.rest = m->rest_joints; pa.feat = p.feat; pa.A = p.A;
    pa.joints = joints; pa.n = n; pa.is_rotmat = pose_is_rotmat ? 1 : 0; pa.NB = m->NB; pa.K = p.rows; pa.KP = p.KP; pa.tree = p.tree;
    hipLaunchKernelGGL(pgsm::smpl_pre_kernel, dim3((unsigned)((n + pgsm::WAVES - 1) / pgsm::WAVES)), dim3(pgsm::THREADS), 0, st, pa);
    PG_LAUNCH_CHECK(h, "body model pose kernel");
    return PG_OK;
}

}  // namespace

extern "C" int pg_smpl_forward(pg_handle* h, void* stream, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride,
                               const float* pose, int pose_is_rotmat, const float* regress, int K, float* verts, float* joints,
                               float* regressed) {
    BodyPlan p;
    PG_TRY(body_plan(h, "pg_smpl_forward", m, B, betas, betas_stride, pose, regress, K,
                     !verts && !joints && !regressed ? "no output asked for" : nullptr, regressed ? "regressed asked for" : nullptr, p));
    const int V = m->V, KR = regressed ? K : 0;
    const bool body = verts || regressed;
    const int chunks = p.tiles < pgsm::MAX_CHUNKS ? p.tiles : pgsm::MAX_CHUNKS;
    long long S = body ? slice_poses(((size_t)p.KP + pgsm::NJ * 12) * sizeof(float) + (size_t)chunks * KR * 3 * sizeof(double), pgsm::WS_TARGET) : B;
    if (S > B) S = B;

    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (body) PG_TRY(carve_body(h, p, (size_t)chunks * S * KR * 3, S));

    for (long long b0 = 0; b0 < B; b0 += S) {
        const long long n = B - b0 < S ? B - b0 : S;
        PG_TRY(launch_pre(h, st, p, m, betas + b0 * betas_stride, betas_stride, pose + (size_t)b0 * pgsm::NJ * (pose_is_rotmat ? 9 : 3),
                          pose_is_rotmat, joints ? joints + (size_t)b0 * pgsm::NJ * 3 : nullptr, n));
        if (!body) continue;
        pgsm::BodyArgs ba{};
        ba.blend = m->blend; ba.skin = m->skin; ba.regress = regress; ba.feat = p.feat; ba.A = p.A;
        ba.verts = verts ? verts + (size_t)b0 * V * 3 : nullptr;
        ba.part = p.part; ba.n = n; ba.V = V; ba.K = p.rows; ba.KP = p.KP; ba.KR = KR; ba.chunks = chunks; ba.tiles = p.tiles;
        hipLaunchKernelGGL(pgsm::smpl_body_kernel, dim3((unsigned)chunks, (unsigned)((n + pgsm::PT - 1) / pgsm::PT)), dim3(pgsm::THREADS), 0, st,
                           ba);
        PG_LAUNCH_CHECK(h, "body model kernel");
        if (KR > 0) {
            const long long per_chunk = n * KR * 3;
            hipLaunchKernelGGL(pgsm::smpl_regress_sum, dim3((unsigned)((per_chunk + pgsm::THREADS - 1) / pgsm::THREADS)), dim3(pgsm::THREADS), 0,
                               st, p.part, per_chunk, chunks, regressed + (size_t)b0 * KR * 3);
            PG_LAUNCH_CHECK(h, "body model regressor sum kernel");
        }
    }
    return PG_OK;
}

extern "C" int pg_smpl_backward(pg_handle* h, void* stream, const pg_body_model* m, int64_t B, const float* betas, int64_t betas_stride,
                                const float* pose, int pose_is_rotmat, const float* regress, int K, const float* blend_t,
                                const float* d_verts, const float* d_joints, const float* d_regressed, float* d_betas, float* d_pose) {
    BodyPlan p;
    PG_TRY(body_plan(h, "pg_smpl_backward", m, B, betas, betas_stride, pose, regress, K,
                     !d_verts && !d_joints && !d_regressed ? "no cotangent given" : !d_betas && !d_pose ? "no output asked for" : nullptr,
                     d_regressed ? "d_regressed given" : nullptr, p));
    const int V = m->V, KR = d_regressed ? K : 0;
    const bool body = d_verts || d_regressed;            // with d_joints alone no vertex-tile kernel runs
    const int chunks = !body ? 0 : p.tiles < pgsm::BWD_MAX_CHUNKS ? p.tiles : pgsm::BWD_MAX_CHUNKS;
    long long S = B;
    if (body) {
        S = slice_poses(((size_t)p.KP + pgsm::NJ * 12) * sizeof(float) + (size_t)chunks * pgsm::BWD_PART * sizeof(double), pgsm::BWD_WS_TARGET);
        // the kernel's LDS admits one workgroup per CU, so a slice of more workgroups than CUs is cut to a whole number of rounds of them
        const long long wgs = S / pgsm::PT * chunks, cus = h->n_cu > 0 ? h->n_cu : 256;
        const long long whole = wgs / cus * cus / chunks;          // pose tiles of the whole rounds
        if (whole >= 1) S = whole * pgsm::PT;
    }
    if (S > B) S = B;

    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (body) PG_TRY(carve_body(h, p, (size_t)chunks * S * pgsm::BWD_PART, S));

    for (long long b0 = 0; b0 < B; b0 += S) {
        const long long n = B - b0 < S ? B - b0 : S;
        const float* sl_betas = betas + b0 * betas_stride;
        const float* sl_pose = pose + (size_t)b0 * pgsm::NJ * (pose_is_rotmat ? 9 : 3);
        if (body) {
            PG_TRY(launch_pre(h, st, p, m, sl_betas, betas_stride, sl_pose, pose_is_rotmat, nullptr, n));
            pgsm::BwdArgs ba{};
            ba.blend = m->blend; ba.blend_t = blend_t; ba.skin = m->skin; ba.regress = regress; ba.feat = p.feat; ba.A = p.A;
            ba.d_verts = d_verts ? d_verts + (size_t)b0 * V * 3 : nullptr;
            ba.d_reg = d_regressed ? d_regressed + (size_t)b0 * KR * 3 : nullptr;
            ba.part = p.part; ba.n = n; ba.V = V; ba.K = p.rows; ba.KP = p.KP; ba.KR = KR; ba.chunks = chunks; ba.tiles = p.tiles;
            hipLaunchKernelGGL(pgsm::smpl_body_bwd_kernel, dim3((unsigned)chunks, (unsigned)((n + pgsm::PT - 1) / pgsm::PT)), dim3(pgsm::THREADS),
                               0, st, ba);
            PG_LAUNCH_CHECK(h, "body model backward kernel");
        }
        pgsm::CloseArgs ca{};
        ca.betas = sl_betas; ca.betas_stride = betas_stride; ca.pose = sl_pose; ca.rest = m->rest_joints; ca.part = p.part;
        ca.d_joints = d_joints ? d_joints + (size_t)b0 * pgsm::NJ * 3 : nullptr;
        ca.d_betas = d_betas ? d_betas + (size_t)b0 * m->NB : nullptr;
        ca.d_pose = d_pose ? d_pose + (size_t)b0 * pgsm::NJ * (pose_is_rotmat ? 9 : 3) : nullptr;
        ca.n = n; ca.is_rotmat = pose_is_rotmat ? 1 : 0; ca.NB = m->NB; ca.chunks = chunks; ca.tree = p.tree;
        hipLaunchKernelGGL(pgsm::smpl_close_kernel, dim3((unsigned)((n + pgsm::WAVES - 1) / pgsm::WAVES)), dim3(pgsm::THREADS), 0, st, ca);
        PG_LAUNCH_CHECK(h, "body model backward closing kernel");
    }
    return PG_OK;
}

extern "C" int pg_vertex_errors(pg_handle* h, void* stream, int64_t B, int V, const float* a, const float* b, double* per_pose,
                                double* summary) {
    const char* who = "pg_vertex_errors";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!a || !b || !per_pose) return pg_fail(h, PG_EINVAL, "%s: a, b and per_pose are required", who);
    if (B < 1 || V < 1) return pg_fail(h, PG_EINVAL, "%s: B = %lld, V = %d", who, (long long)B, V);
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pgsm::vertex_err_kernel, dim3((unsigned)((B + pgsm::WAVES - 1) / pgsm::WAVES)), dim3(pgsm::THREADS), 0, st, a, b,
                       (long long)B, V, per_pose);
    PG_LAUNCH_CHECK(h, "vertex error kernel");
    if (summary) {
        hipLaunchKernelGGL(pgsm::vertex_err_mean, dim3(1), dim3(pgsm::THREADS), 0, st, per_pose, (long long)B, summary);
        PG_LAUNCH_CHECK(h, "vertex error mean kernel");
    }
    return PG_OK;
}

extern "C" int pg_pose_kinematics_rot(pg_handle* h, void* stream, int64_t n_poses, const float* rotmats, const double* bone_offsets,
                                      const int32_t* parents, float* kps, float* skts, double* l2ws) {
    const char* who = "pg_pose_kinematics_rot";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_poses < 0 || !rotmats || !bone_offsets || !parents) return pg_fail(h, PG_EINVAL, "%s: null/negative argument", who);
    pgsm::KinConst kc;
    if (parents[0] != -1 || !pgkin::pg_kin_tree(parents, kc.tree))
        return pg_fail(h, PG_EINVAL, "%s: parents[0] must be -1 and every joint must come after its parent", who);
    if (n_poses == 0) return PG_OK;
    for (int i = 0; i < pgsm::NJ * 3; ++i) kc.offs[i] = bone_offsets[i];
    PG_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(pgsm::kin_rot_kernel, dim3((unsigned)((n_poses + pgsm::WAVES - 1) / pgsm::WAVES)), dim3(pgsm::THREADS), 0,
                       static_cast<hipStream_t>(stream), kc, rotmats, (long long)n_poses, kps, skts, l2ws);
    PG_LAUNCH_CHECK(h, "rotation-matrix kinematics kernel");
    return PG_OK;
}
