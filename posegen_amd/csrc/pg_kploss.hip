// pg_kploss.hip -- training on pose error: the transposes of the two key-point kinematics for their `kps` output, and
// the two pose losses of the GAN loop with their gradients.
//   kin_bwd_kernel<AXIS> : the transpose of pose_kinematics_kernel (pg_kernels.hip; AXIS, axis-angle float64 in, float64 out) and of
//                          kin_rot_kernel (pg_smpl.hip; nine free matrix entries, float32 in and out).  One wave per pose, lane =
//                          joint.  The forward again from the parameters -- relative transforms and the chain product level by
//                          level in LDS -- then the cotangent of every joint's l2w rows (only column 3, the key point, is fed) walked
//                          back up the tree, a parent collecting its children in joint order, then dR_j = R_parent^T G_j and, for
//                          AXIS, matrix -> unit quaternion -> rotation vector transposed.  Below theta = 1e-3 that last step is the
//                          derivative of the series in theta^2 (k = 1/2 - t/48 + t^2/3840, q_w = 1 - t/8 + t^2/384), finite at zero.
//   loss_pose_kernel     : run_gan.py:1898-1906 / mpjpe (:1458-1464) per pose: one wave per pose, lane = selected joint; rows
//                          `joints` minus row `root` in double, optionally the prediction rescaled to the ground truth's Frobenius
//                          norm, weight times the mean joint distance -> vals[b].
//   loss_sum_kernel      : the kept set (vals[b] < cap, strict; everything under cap = +inf) and loss = sum kept / n_kept in a fixed
//                          order -> summary[3]; one workgroup.
//   loss_grad_kernel     : the gradients of `loss` at upstream 1 -> d_pred / d_gt [B,J_in,3]; one wave per pose.  Every row is
//                          written once, by one lane: selected rows get their lane's value by a wave shuffle, the root row minus the
//                          sum of them, the others and the poses that are not kept zero.
// float64 arithmetic, outputs rounded once; no atomics, every sum in a fixed order; nothing is kept between calls.  The chain, its
// transpose and the rotation-vector map with its transpose are pg_kin.h's, shared with the forward kernels they belong to.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pg_handle.h"
#include "pg_kin.h"

namespace pgkl {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAXJ = 64;

using pgkin::KinConst;
using pgkin::NJ;
using pgkin::wave_all_sum;

// One wave per pose, lane = joint.  `in`: bones [n,24,3] double (AXIS) or rotmats [n,24,3,3] float; `out`: the same shape and type.
template <bool AXIS>
__global__ __launch_bounds__(THREADS) void kin_bwd_kernel(const KinConst kc, const void* __restrict__ in, long long n,
                                                          const float* __restrict__ d_kps, void* __restrict__ out) {
    __shared__ double rel[WAVES][NJ][12], l2w[WAVES][NJ][12], G[WAVES][NJ][12];
    __shared__ int spar[NJ], slev[NJ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < NJ) { spar[threadIdx.x] = kc.tree.parent[threadIdx.x]; slev[threadIdx.x] = kc.tree.level[threadIdx.x]; }
    long long pose = (long long)blockIdx.x * WAVES + w;
    const bool live = pose < n;
    if (!live) pose = n - 1;                                 // (a wave past the end walks the last pose again and writes nothing)
    const bool jl = lane < NJ;
    const int j = jl ? lane : 0;
    const size_t at = (size_t)pose * NJ + j;

    // 1. the forward: the joint's relative transform, then the chain level by level
    pgkin::Quat s;
    double R[12];
    if constexpr (AXIS) {
        pgkin::rotvec_to_rows(static_cast<const double*>(in) + at * 3, s, R);
    } else {
        pgkin::rotmat_to_rows(static_cast<const float*>(in) + at * 9, R);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) R[4 * r + 3] = kc.offs[3 * j + r];
    __syncthreads();                                         // spar / slev
    const int par = spar[j], lev = slev[j];
    if (jl) {                                                // the cotangent of the l2w rows: only column 3, the key point, is fed
#pragma unroll
        for (int e = 0; e < 12; ++e) G[w][j][e] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) G[w][j][4 * r + 3] = (double)d_kps[at * 3 + r];
    }
    pgkin::chain_forward(rel[w], l2w[w], R, j, jl, par, lev, kc.tree.depth);       // (its first barrier covers G)
    // 2. the chain backwards, children before parents
    pgkin::chain_backward(G[w], rel[w], spar, j, jl, lev, kc.tree.depth);
    if (!live || !jl) return;
    // 3. dR_j = (l2w_parent^T G_j)[:3,:3] (the root's parent is the identity)
    double D[9];
    pgkin::parent_transpose<3>(l2w[w], par, G[w][j], D);
    if constexpr (AXIS) {
        double o[3];
        pgkin::rotvec_bwd(s, D, o);
        double* dst = static_cast<double*>(out) + at * 3;
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    } else {
        float* dst = static_cast<float*>(out) + at * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) dst[e] = (float)D[e];
    }
}

// ---- the losses ---------------------------------------------------------------------------------------------------------------------
struct LossArgs {
    const float* pred;
    const float* gt;
    long long B;
    int J_in, J, root, kind;
    double weight, cap;
    double* vals;                // [B]: weight e_b
    const double* summary;       // loss_grad_kernel: n_kept at [1]
    float* d_pred;
    float* d_gt;
    int32_t joints[MAXJ];
};

// What a lane holds of its pose: the centred joint of both sets, the residual e = s p - g with its length, and the pose's norms.
struct PoseTerm {
    double p[3], g[3], e[3], dist;
    double s, pp, np, ng;        // scale, |p|_F^2, |p|_F, |g|_F
};

__device__ __forceinline__ void pose_term(const LossArgs& a, long long pose, int lane, PoseTerm& t) {
    const bool live = lane < a.J;
    const int row = live ? a.joints[lane] : 0;
    const float* pp = a.pred + ((size_t)pose * a.J_in) * 3;
    const float* gp = a.gt + ((size_t)pose * a.J_in) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t.p[c] = live ? (double)pp[(size_t)row * 3 + c] : 0.0;
        t.g[c] = live ? (double)gp[(size_t)row * 3 + c] : 0.0;
        if (a.root >= 0 && live) { t.p[c] -= (double)pp[(size_t)a.root * 3 + c]; t.g[c] -= (double)gp[(size_t)a.root * 3 + c]; }
    }
    t.s = 1.0; t.pp = 0.0; t.np = 0.0; t.ng = 0.0;
    if (a.kind == PG_POSE_LOSS_NORM_MATCHED) {
        t.pp = wave_all_sum(t.p[0] * t.p[0] + t.p[1] * t.p[1] + t.p[2] * t.p[2]);
        t.np = sqrt(t.pp);
        t.ng = sqrt(wave_all_sum(t.g[0] * t.g[0] + t.g[1] * t.g[1] + t.g[2] * t.g[2]));
        t.s = t.ng / t.np;                                   // |p| = 0: inf or NaN, and the pose NaN with it (inf 0)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) t.e[c] = t.s * t.p[c] - t.g[c];
    t.dist = live ? sqrt(t.e[0] * t.e[0] + t.e[1] * t.e[1] + t.e[2] * t.e[2]) : 0.0;
}

__global__ __launch_bounds__(THREADS) void loss_pose_kernel(LossArgs a) {
    const int lane = threadIdx.x & 63;
    const long long pose = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (pose >= a.B) return;                                 // (a whole wave leaves: the shuffles below keep all 64 lanes)
    PoseTerm t;
    pose_term(a, pose, lane, t);
    const double e = wave_all_sum(t.dist) / (double)a.J;
    if (lane == 0) a.vals[pose] = a.weight * e;
}

__device__ __forceinline__ bool kept(double v, double cap) { return cap == INFINITY || v < cap; }

// summary = loss, n_kept, B.  Thread t adds poses t, t + 256, ... in that order; the 256 partial sums fold in a fixed tree.
__global__ __launch_bounds__(THREADS) void loss_sum_kernel(const double* __restrict__ vals, long long B, double cap, double* __restrict__ summary) {
    __shared__ double ssum[THREADS];
    __shared__ long long scnt[THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    long long cnt = 0;
    for (long long b = tid; b < B; b += THREADS) {
        const double v = vals[b];
        if (kept(v, cap)) { acc += v; ++cnt; }
    }
    ssum[tid] = acc; scnt[tid] = cnt;
    __syncthreads();
    for (int d = THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) { ssum[tid] += ssum[tid + d]; scnt[tid] += scnt[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) {
        summary[0] = ssum[0] / (double)scnt[0];             // nothing kept: 0 / 0, torch.mean of an empty tensor
        summary[1] = (double)scnt[0];
        summary[2] = (double)B;
    }
}

__global__ __launch_bounds__(THREADS) void loss_grad_kernel(LossArgs a) {
    const int lane = threadIdx.x & 63;
    const long long pose = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (pose >= a.B) return;
    const bool live = lane < a.J;
    const double n_kept = a.summary[1];
    double dp[3] = {0.0, 0.0, 0.0}, dg[3] = {0.0, 0.0, 0.0};
    if (kept(a.vals[pose], a.cap)) {                         // (uniform over the wave)
        PoseTerm t;
        pose_term(a, pose, lane, t);
        const double c = a.weight / ((double)a.J * n_kept);
        double u[3] = {0.0, 0.0, 0.0};
        if (live && t.dist != 0.0) {                         // a zero distance: a zero gradient, as torch's norm backward gives
#pragma unroll
            for (int k = 0; k < 3; ++k) u[k] = t.e[k] / t.dist;
        }
        if (a.kind == PG_POSE_LOSS_NORM_MATCHED) {
            const double al = wave_all_sum(u[0] * t.p[0] + u[1] * t.p[1] + u[2] * t.p[2]);
            const double fp = t.s * al / t.pp;
            const double fg = t.ng != 0.0 ? al / (t.np * t.ng) : 0.0;        // |g| = 0: torch's norm backward gives zero there too
#pragma unroll
            for (int k = 0; k < 3; ++k) { dp[k] = c * (t.s * u[k] - fp * t.p[k]); dg[k] = c * (-u[k] + fg * t.g[k]); }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { dp[k] = c * u[k]; dg[k] = -c * u[k]; }
        }
        if (!live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { dp[k] = 0.0; dg[k] = 0.0; }
        }
    }
    double rp[3], rg[3];                                     // the root row's share: minus the sum of the selected rows
#pragma unroll
    for (int k = 0; k < 3; ++k) { rp[k] = -wave_all_sum(dp[k]); rg[k] = -wave_all_sum(dg[k]); }
    // every row of the pose once: row r belongs to lane r0 + lane, its value sits in the lane that selected it
    for (int r0 = 0; r0 < a.J_in; r0 += 64) {
        const int r = r0 + lane;
        int src = -1;
        for (int q = 0; q < a.J; ++q)
            if (a.joints[q] == r) src = q;
        const bool sel = src >= 0;
        double vp[3], vg[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            vp[k] = __shfl(dp[k], sel ? src : 0);
            vg[k] = __shfl(dg[k], sel ? src : 0);
            if (!sel) { vp[k] = 0.0; vg[k] = 0.0; }
            if (r == a.root) { vp[k] += rp[k]; vg[k] += rg[k]; }
        }
        if (r < a.J_in) {
            const size_t o = ((size_t)pose * a.J_in + r) * 3;
            if (a.d_pred) { a.d_pred[o] = (float)vp[0]; a.d_pred[o + 1] = (float)vp[1]; a.d_pred[o + 2] = (float)vp[2]; }
            if (a.d_gt) { a.d_gt[o] = (float)vg[0]; a.d_gt[o + 1] = (float)vg[1]; a.d_gt[o + 2] = (float)vg[2]; }
        }
    }
}

}  // namespace pgkl

// ---- the host side --------------------------------------------------------------------------------------------------------------------
namespace {

// the per-pose values of a pg_pose_loss call that passes no per_pose.  One buffer per handle: calls on one handle are serialised by
// the caller (as pg_posescore.hip).
struct KpLossState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_KPLOSS;
    ~KpLossState() override { pg_release(vals); }
    DevBuf vals;
};
static_assert(pgkl::MAXJ == PG_POSE_MAX_JOINTS, "pg_check_joint_selection bounds J for the kernel's joint table");

template <bool AXIS>
int kin_bwd(pg_handle* h, const char* who, void* stream, int64_t n_poses, const void* in, const double* bone_offsets, const int32_t* parents,
            const float* d_kps, void* out) {
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_poses < 0 || !in || !bone_offsets || !parents || !d_kps || !out) return pg_fail(h, PG_EINVAL, "%s: null/negative argument", who);
    if (n_poses > 0x7fffffffll * pgkl::WAVES) return pg_fail(h, PG_EINVAL, "%s: n_poses = %lld", who, (long long)n_poses);
    pgkl::KinConst kc;
    // the root's own entry: 0 in the skeleton's table, -1 in a body model's, and both are taken
    if ((parents[0] != 0 && parents[0] != -1) || !pgkin::pg_kin_tree(parents, kc.tree))
        return pg_fail(h, PG_EINVAL, "%s: every joint must come after its parent", who);
    if (n_poses == 0) return PG_OK;
    for (int i = 0; i < pgkl::NJ * 3; ++i) kc.offs[i] = bone_offsets[i];
    PG_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(pgkl::kin_bwd_kernel<AXIS>, dim3((unsigned)((n_poses + pgkl::WAVES - 1) / pgkl::WAVES)), dim3(pgkl::THREADS), 0,
                       static_cast<hipStream_t>(stream), kc, in, (long long)n_poses, d_kps, out);
    PG_LAUNCH_CHECK(h, "kinematics backward kernel");
    return PG_OK;
}

}  // namespace

extern "C" int pg_pose_kinematics_bwd(pg_handle* h, void* stream, int64_t n_poses, const double* bones, const double* bone_offsets,
                                      const int32_t* parents, const float* d_kps, double* d_bones) {
    return kin_bwd<true>(h, "pg_pose_kinematics_bwd", stream, n_poses, bones, bone_offsets, parents, d_kps, d_bones);
}

extern "C" int pg_pose_kinematics_rot_bwd(pg_handle* h, void* stream, int64_t n_poses, const float* rotmats, const double* bone_offsets,
                                          const int32_t* parents, const float* d_kps, float* d_rotmats) {
    return kin_bwd<false>(h, "pg_pose_kinematics_rot_bwd", stream, n_poses, rotmats, bone_offsets, parents, d_kps, d_rotmats);
}

extern "C" int pg_pose_loss(pg_handle* h, void* stream, int64_t B, int J_in, const float* pred, const float* gt, const int32_t* joints, int J,
                            int root, int kind, double weight, double cap, double* per_pose, double* summary, float* d_pred, float* d_gt) {
    const char* who = "pg_pose_loss";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!pred || !gt || !summary) return pg_fail(h, PG_EINVAL, "%s: pred, gt and summary are required", who);
    if (B < 1 || B > 0x7fffffffll * pgkl::WAVES) return pg_fail(h, PG_EINVAL, "%s: B = %lld", who, (long long)B);
    PG_TRY(pg_check_joint_selection(h, who, J_in, joints, &J, root, true));
    if (kind != PG_POSE_LOSS_MPJPE && kind != PG_POSE_LOSS_NORM_MATCHED) return pg_fail(h, PG_EINVAL, "%s: unknown kind %d", who, kind);
    if (std::isnan(weight) || std::isnan(cap) || cap <= 0.0) return pg_fail(h, PG_EINVAL, "%s: weight = %g, cap = %g (no NaN; cap > 0)", who, weight, cap);
    if (pg_misaligned(pred, sizeof(float)) || pg_misaligned(gt, sizeof(float)) || pg_misaligned(d_pred, sizeof(float)) ||
        pg_misaligned(d_gt, sizeof(float)) || pg_misaligned(per_pose, sizeof(double)) || pg_misaligned(summary, sizeof(double)))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);

    PG_HIP(h, hipSetDevice(h->device));
    double* vals = per_pose;
    if (!vals) {
        KpLossState* s = nullptr;
        PG_TRY(pg_state(h, s));
        PG_TRY(pg_grow(h, s->vals, (size_t)B * sizeof(double), "pose loss values", (size_t)(B + B / 2) * sizeof(double)));
        vals = s->vals.as<double>();
    }
    pgkl::LossArgs a{};
    a.pred = pred; a.gt = gt; a.B = B; a.J_in = J_in; a.J = J; a.root = root; a.kind = kind; a.weight = weight; a.cap = cap;
    a.vals = vals; a.summary = summary; a.d_pred = d_pred; a.d_gt = d_gt;
    for (int j = 0; j < pgkl::MAXJ; ++j) a.joints[j] = j < J ? (joints ? joints[j] : j) : -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((B + pgkl::WAVES - 1) / pgkl::WAVES));
    hipLaunchKernelGGL(pgkl::loss_pose_kernel, grid, dim3(pgkl::THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "pose loss kernel");
    hipLaunchKernelGGL(pgkl::loss_sum_kernel, dim3(1), dim3(pgkl::THREADS), 0, st, vals, (long long)B, cap, summary);
    PG_LAUNCH_CHECK(h, "pose loss sum kernel");
    if (d_pred || d_gt) {
        hipLaunchKernelGGL(pgkl::loss_grad_kernel, grid, dim3(pgkl::THREADS), 0, st, a);
        PG_LAUNCH_CHECK(h, "pose loss gradient kernel");
    }
    return PG_OK;
}
