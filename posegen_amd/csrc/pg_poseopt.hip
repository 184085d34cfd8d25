// pg_poseopt.hip -- the pose layer of pose refinement on the device: the reference's PoseOptLayer.calculate_kinematic
// (core/pose_opt.py:372-445) in the configuration its shipped configs train with (SMPL skeleton, use_rot6d, no cache), forward and
// backward, behind pg_poseopt_forward / pg_poseopt_backward (include/posegen_hip.h).
//
//   forward, per unique pose u (pose_opt.py:391-445):
//     R_j   = rot6d_to_rotmat(bones[u][j])                       (skeleton_utils.py:507-523: two F.normalize, one cross product)
//     rel_j = [R_j | rest[j] - rest[parent j]]  (root: [R | rest[root]]);   l2w_j = l2w_parent(j) rel_j      (pose_opt.py:399-414;
//             the levels of unrolled_kinematic_chain, pose_opt.py:482-521, are the depth levels of the joint tree)
//     l2w_j[:3,3] += pelvis[u];   skt_j = l2w_j^-1;   kp_j = l2w_j[:3,3]                                     (pose_opt.py:423-443)
//   and the results written once per ray of the pose (the reference's gather by inverse_idxs, pose_opt.py:438-441).
//
//   backward: the forward of the pose again from the parameters (nothing is kept between the two calls), then the transpose of
//   every step above.  The per-ray cotangents of a pose are summed in ASCENDING RAY ORDER by one thread per entry -- the reference
//   sums them in the backward of skts[inverse_idxs], an atomic scatter-add in no fixed order on a GPU -- so the parameter
//   gradients are bitwise repeatable (the rule of sc_partial_kernel / reduce_parts_kernel: fixed order, no atomics).
//
// Arithmetic: float64 inside, float32 in and out (rounded once).  One workgroup per pose; the joint tree is walked level by level
// with the pose's matrices in LDS (lane = joint; chain_forward / chain_backward, pg_kin.h).  The work is a few hundred poses of 24
// joints: its cost is the launch.
#include <hip/hip_runtime.h>

#include <vector>

#include "pg_handle.h"
#include "pg_kin.h"

namespace pgp {

using pgkin::NJ;
constexpr int THREADS = 256;
constexpr int N_ROT = NJ * 9, N_MAT = NJ * 16, N_KP = NJ * 3;
constexpr double EPS = 1e-12;          // F.normalize's eps (skeleton_utils.py:520-521)

// what one joint's 6-D -> matrix map leaves for its transpose
struct Rot6 {
    double b1[3], b2[3], b3[3], a2[3];
    double n1, n2, s;                   // |a1|, |a2 - (b1 . a2) b1|, b1 . a2
};

__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// rot6d_to_rotmat (skeleton_utils.py:507-523): x viewed as [3,2], a1 = column 0, a2 = column 1
__device__ inline void rot6d(const float* __restrict__ x, Rot6& q) {
    const double a1[3] = {(double)x[0], (double)x[2], (double)x[4]};
    q.a2[0] = (double)x[1]; q.a2[1] = (double)x[3]; q.a2[2] = (double)x[5];
    q.n1 = sqrt(dot3(a1, a1));
    const double d1 = fmax(q.n1, EPS);
    for (int i = 0; i < 3; ++i) q.b1[i] = a1[i] / d1;
    q.s = dot3(q.b1, q.a2);
    double u2[3];
    for (int i = 0; i < 3; ++i) u2[i] = q.a2[i] - q.s * q.b1[i];
    q.n2 = sqrt(dot3(u2, u2));
    const double d2 = fmax(q.n2, EPS);
    for (int i = 0; i < 3; ++i) q.b2[i] = u2[i] / d2;
    cross3(q.b1, q.b2, q.b3);
}

// Rows 0..2 of every joint's relative transform and of its chain product WITHOUT the pelvis shift (pose_opt.py:399-414), in LDS.
// Called by every thread of the workgroup (barriers inside); lanes 0..23 are the joints (j: the thread's, 0 for the others).
// parent / level: LDS copies of the tree.
__device__ inline void pose_chain(int u, int j, bool jl, const float* __restrict__ bones, const float* __restrict__ rest, int rest_stride,
                                  const int* parent, const int* level, int max_depth, double (*rel)[12], double (*l2w)[12], Rot6& q) {
    const int p = parent[j];
    double R[12];
    if (jl) {
        rot6d(bones + ((long long)u * NJ + j) * 6, q);
        const float* rp = rest + (long long)u * rest_stride;
        for (int r = 0; r < 3; ++r) {
            R[4 * r] = q.b1[r]; R[4 * r + 1] = q.b2[r]; R[4 * r + 2] = q.b3[r];
            R[4 * r + 3] = p < 0 ? (double)rp[3 * j + r] : (double)rp[3 * j + r] - (double)rp[3 * p + r];
        }
    }
    pgkin::chain_forward(rel, l2w, R, j, jl, p, level[j], max_depth);
}

// rows 0..2 of m^-1 for m = [A | t; 0 0 0 1] given as its rows 0..2 (pose_opt.py:435, torch.inverse): [A^-1 | -A^-1 t]
__device__ inline void inverse_rows(const double* m, double* s) {
    const double c00 = m[5] * m[10] - m[6] * m[9], c01 = m[6] * m[8] - m[4] * m[10], c02 = m[4] * m[9] - m[5] * m[8];
    const double inv = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
    s[0] = c00 * inv; s[1] = (m[2] * m[9] - m[1] * m[10]) * inv; s[2] = (m[1] * m[6] - m[2] * m[5]) * inv;
    s[4] = c01 * inv; s[5] = (m[0] * m[10] - m[2] * m[8]) * inv; s[6] = (m[2] * m[4] - m[0] * m[6]) * inv;
    s[8] = c02 * inv; s[9] = (m[1] * m[8] - m[0] * m[9]) * inv;  s[10] = (m[0] * m[5] - m[1] * m[4]) * inv;
    for (int r = 0; r < 3; ++r) s[4 * r + 3] = -(s[4 * r] * m[3] + s[4 * r + 1] * m[7] + s[4 * r + 2] * m[11]);
}

__device__ inline void load_tree(int tid, const int* __restrict__ tree, int* parent, int* level) {
    if (tid < NJ) { parent[tid] = tree[tid]; level[tid] = tree[NJ + tid]; }
    __syncthreads();
}

// One workgroup per pose.  seg_start [U+1] / seg_rays [n]: the rays of every pose (null: ray u is pose u).
__global__ __launch_bounds__(THREADS) void poseopt_fwd_kernel(const float* __restrict__ bones, const float* __restrict__ pelvis,
                                                              const float* __restrict__ rest, int rest_stride, const int* __restrict__ tree,
                                                              int max_depth, const int* __restrict__ seg_start, const int* __restrict__ seg_rays,
                                                              float* __restrict__ rots, float* __restrict__ l2ws, float* __restrict__ skts,
                                                              float* __restrict__ kps) {
    __shared__ double rel[NJ][12], l2w[NJ][12];
    __shared__ float o_rot[N_ROT], o_l2w[N_MAT], o_skt[N_MAT], o_kp[N_KP];
    __shared__ int parent[NJ], level[NJ];
    const int u = blockIdx.x, tid = threadIdx.x;
    const bool jl = tid < NJ;
    const int j = jl ? tid : 0;
    load_tree(tid, tree, parent, level);
    Rot6 q;
    pose_chain(u, j, jl, bones, rest, rest_stride, parent, level, max_depth, rel, l2w, q);
    if (tid < NJ) {
        double m[12], s[12];
        for (int e = 0; e < 12; ++e) m[e] = l2w[tid][e];
        for (int r = 0; r < 3; ++r) m[4 * r + 3] += (double)pelvis[(long long)u * 3 + r];        // pose_opt.py:423-432
        inverse_rows(m, s);
        for (int r = 0; r < 3; ++r) {
            o_rot[9 * tid + 3 * r] = (float)q.b1[r]; o_rot[9 * tid + 3 * r + 1] = (float)q.b2[r]; o_rot[9 * tid + 3 * r + 2] = (float)q.b3[r];
            o_kp[3 * tid + r] = (float)m[4 * r + 3];
        }
        for (int e = 0; e < 12; ++e) { o_l2w[16 * tid + e] = (float)m[e]; o_skt[16 * tid + e] = (float)s[e]; }
        for (int e = 12; e < 16; ++e) { o_l2w[16 * tid + e] = e == 15 ? 1.f : 0.f; o_skt[16 * tid + e] = e == 15 ? 1.f : 0.f; }
    }
    __syncthreads();
    const int i0 = seg_start ? seg_start[u] : u, i1 = seg_start ? seg_start[u + 1] : u + 1;
    for (int i = i0; i < i1; ++i) {
        const long long r = seg_rays ? seg_rays[i] : i;
        if (rots) for (int e = tid; e < N_ROT; e += THREADS) rots[r * N_ROT + e] = o_rot[e];
        if (l2ws) for (int e = tid; e < N_MAT; e += THREADS) l2ws[r * N_MAT + e] = o_l2w[e];
        if (skts) for (int e = tid; e < N_MAT; e += THREADS) skts[r * N_MAT + e] = o_skt[e];
        if (kps) for (int e = tid; e < N_KP; e += THREADS) kps[r * N_KP + e] = o_kp[e];
    }
}

// the sum of one entry of a per-ray cotangent over the pose's rays, in ascending ray order (null: zero)
__device__ inline double segment_sum(const float* __restrict__ src, int per_ray, int e, const int* __restrict__ seg_rays, int i0, int i1) {
    double acc = 0.0;
    if (src)
        for (int i = i0; i < i1; ++i) acc += (double)src[(long long)seg_rays[i] * per_ray + e];
    return acc;
}

// the transpose of v / max(|v|, eps) (F.normalize): b the normalised vector, n = |v|, g the cotangent of b
__device__ inline void normalize_bwd(const double* b, double n, const double* g, double* o) {
    if (n > EPS) {
        const double t = dot3(b, g);
        for (int i = 0; i < 3; ++i) o[i] = (g[i] - b[i] * t) / n;
    } else {
        for (int i = 0; i < 3; ++i) o[i] = g[i] / EPS;
    }
}

__global__ __launch_bounds__(THREADS) void poseopt_bwd_kernel(const float* __restrict__ bones, const float* __restrict__ pelvis,
                                                              const float* __restrict__ rest, int rest_stride, const int* __restrict__ tree,
                                                              int max_depth, const int* __restrict__ seg_start, const int* __restrict__ seg_rays,
                                                              const float* __restrict__ d_rots, const float* __restrict__ d_l2ws,
                                                              const float* __restrict__ d_skts, const float* __restrict__ d_kps,
                                                              float* __restrict__ d_bones, float* __restrict__ d_pelvis) {
    __shared__ double rel[NJ][12], l2w[NJ][12], G[NJ][12];
    __shared__ double c_rot[N_ROT], c_l2w[N_MAT], c_skt[N_MAT], c_kp[N_KP];
    __shared__ double pel[NJ][3];
    __shared__ int parent[NJ], level[NJ];
    const int u = blockIdx.x, tid = threadIdx.x;
    const bool jl = tid < NJ;
    const int j = jl ? tid : 0;
    load_tree(tid, tree, parent, level);
    // 1. the ordered segment sums: one thread per entry
    const int i0 = seg_start[u], i1 = seg_start[u + 1];
    for (int e = tid; e < N_ROT; e += THREADS) c_rot[e] = segment_sum(d_rots, N_ROT, e, seg_rays, i0, i1);
    for (int e = tid; e < N_MAT; e += THREADS) c_l2w[e] = segment_sum(d_l2ws, N_MAT, e, seg_rays, i0, i1);
    for (int e = tid; e < N_MAT; e += THREADS) c_skt[e] = segment_sum(d_skts, N_MAT, e, seg_rays, i0, i1);
    for (int e = tid; e < N_KP; e += THREADS) c_kp[e] = segment_sum(d_kps, N_KP, e, seg_rays, i0, i1);
    Rot6 q;
    pose_chain(u, j, jl, bones, rest, rest_stride, parent, level, max_depth, rel, l2w, q);     // (its first barrier covers the sums)
    if (tid < NJ) {
        // 2. dL2W = -S^T dS S^T (rows 0..2; row 3 of l2w is constant) + d_l2ws, d_kps into column 3
        double m[12], s[12];
        for (int e = 0; e < 12; ++e) m[e] = l2w[tid][e];
        for (int r = 0; r < 3; ++r) m[4 * r + 3] += (double)pelvis[(long long)u * 3 + r];
        inverse_rows(m, s);
        const double* dS = c_skt + 16 * tid;
        for (int r = 0; r < 3; ++r) {
            double T[4];
            for (int k = 0; k < 4; ++k) T[k] = s[r] * dS[k] + s[4 + r] * dS[4 + k] + s[8 + r] * dS[8 + k];
            for (int c = 0; c < 3; ++c)
                G[tid][4 * r + c] = c_l2w[16 * tid + 4 * r + c] - (T[0] * s[4 * c] + T[1] * s[4 * c + 1] + T[2] * s[4 * c + 2] + T[3] * s[4 * c + 3]);
            G[tid][4 * r + 3] = c_l2w[16 * tid + 4 * r + 3] + c_kp[3 * tid + r] - T[3];
            pel[tid][r] = G[tid][4 * r + 3];
        }
    }
    __syncthreads();
    // 3. the pelvis shift reaches column 3 of every joint
    if (tid < 3) {
        double acc = 0.0;
        for (int j = 0; j < NJ; ++j) acc += pel[j][tid];
        d_pelvis[(long long)u * 3 + tid] = (float)acc;
    }
    // 4. the chain backwards, children before parents: a parent collects its children in joint order
    pgkin::chain_backward(G, rel, parent, j, jl, level[j], max_depth);
    if (tid < NJ) {
        // 5. dR = (l2w_parent^T dL2W)[:3,:3] + d_rots (the root's parent is the identity)
        double D[9], dR[9];
        pgkin::parent_transpose<3>(l2w, parent[tid], G[tid], D);
        for (int e = 0; e < 9; ++e) dR[e] = c_rot[9 * tid + e] + D[e];
        // 6. the columns of R are b1, b2, b3 = b1 x b2
        double g1[3], g2[3], g3[3], t[3];
        for (int i = 0; i < 3; ++i) { g1[i] = dR[3 * i]; g2[i] = dR[3 * i + 1]; g3[i] = dR[3 * i + 2]; }
        cross3(q.b2, g3, t);
        for (int i = 0; i < 3; ++i) g1[i] += t[i];
        cross3(g3, q.b1, t);
        for (int i = 0; i < 3; ++i) g2[i] += t[i];
        double du2[3], da1[3], da2[3];
        normalize_bwd(q.b2, q.n2, g2, du2);                 // b2 = normalize(u2), u2 = a2 - s b1, s = b1 . a2
        const double ds = -dot3(du2, q.b1);
        for (int i = 0; i < 3; ++i) {
            da2[i] = du2[i] + ds * q.b1[i];
            g1[i] += -q.s * du2[i] + ds * q.a2[i];
        }
        normalize_bwd(q.b1, q.n1, g1, da1);
        float* o = d_bones + ((long long)u * NJ + tid) * 6;
        for (int i = 0; i < 3; ++i) { o[2 * i] = (float)da1[i]; o[2 * i + 1] = (float)da2[i]; }
    }
}

// what the two entry points keep in the handle: the device copy of the joint tree and of the ray segments, and the host copy the
// upload reads while it is in flight
struct State : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_POSEOPT;
    ~State() override { pg_release(d_idx); }
    DevBuf d_idx;
    std::vector<int32_t> host;
};

constexpr int TREE_WORDS = 64;         // parent [24] (the root's: -1) | level [24] | pad

// the checks both entry points share; fills words [0, 64) of `idx` with the tree, *max_depth with its depth
int check_common(pg_handle* h, const char* who, int64_t n_poses, int rot_dim, const float* bones, const float* pelvis, const float* rest_pose,
                 int64_t rest_stride, const int32_t* parents, int64_t n_rays, std::vector<int32_t>& idx, int* max_depth) {
    if (n_poses < 0 || n_rays < 0 || !bones || !pelvis || !rest_pose || !parents) return pg_fail(h, PG_EINVAL, "%s: null/negative argument", who);
    if (n_poses > 0x7ffffffe || n_rays > 0x7ffffffe) return pg_fail(h, PG_EINVAL, "%s: at most 2^31 - 2 poses / rays per call", who);
    if (h->cfg.n_joints != NJ) return pg_fail(h, PG_EINVAL, "%s: 24-joint SMPL skeleton only", who);
    if (rot_dim != 6) return pg_fail(h, PG_EINVAL, "%s: rot_dim must be 6 (the 6-D rotation parameters of use_rot6d), got %d", who, rot_dim);
    if (rest_stride != 0 && rest_stride != NJ * 3)
        return pg_fail(h, PG_EINVAL, "%s: rest_stride must be 0 (one rest pose) or 72 (one per pose), got %lld", who, (long long)rest_stride);
    idx.assign(TREE_WORDS + (size_t)n_poses + 1 + (size_t)n_rays, 0);
    pgkin::KinTree kt;
    int bad = 0;                        // the root's own entry is 0 here (the skeleton's table)
    if (parents[0] != 0 || !pgkin::pg_kin_tree(parents, kt, &bad))
        return pg_fail(h, PG_EINVAL, "%s: joint %d must come after its parent (%d)", who, bad, parents[bad]);
    for (int j = 0; j < NJ; ++j) { idx[j] = kt.parent[j]; idx[NJ + j] = kt.level[j]; }
    *max_depth = kt.depth;
    return PG_OK;
}

int upload(pg_handle* h, State* s, hipStream_t st) {
    const size_t bytes = s->host.size() * sizeof(int32_t);
    PG_TRY(pg_grow(h, s->d_idx, bytes + bytes / 8, "pose layer index buffer"));
    PG_HIP(h, hipMemcpyAsync(s->d_idx.p, s->host.data(), bytes, hipMemcpyHostToDevice, st));
    return PG_OK;
}

}  // namespace pgp

extern "C" {

int pg_poseopt_forward(pg_handle* h, void* stream, int64_t n_poses, int rot_dim, const float* bones, const float* pelvis,
                       const float* rest_pose, int64_t rest_stride, const int32_t* parents, int64_t n_rays, const int32_t* ray_pose,
                       float* rots, float* l2ws, float* skts, float* kps) {
    using namespace pgp;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    State* s = nullptr;
    PG_TRY(pg_state(h, s));
    int max_depth = 0;
    PG_TRY(check_common(h, "pg_poseopt_forward", n_poses, rot_dim, bones, pelvis, rest_pose, rest_stride, parents, n_rays, s->host, &max_depth));
    if (!ray_pose && n_rays != n_poses)
        return pg_fail(h, PG_EINVAL, "pg_poseopt_forward: without ray_pose ray u is pose u: n_rays (%lld) must equal n_poses (%lld)",
                       (long long)n_rays, (long long)n_poses);
    if (n_poses == 0 || n_rays == 0) return PG_OK;
    const int U = (int)n_poses, n = (int)n_rays;
    int32_t* seg_start = s->host.data() + TREE_WORDS;
    int32_t* seg_rays = seg_start + U + 1;
    if (ray_pose) {
        // the rays of every pose in ascending ray order (a counting sort); an index outside [0, U) never reaches the device
        for (int i = 0; i < n; ++i) {
            if (ray_pose[i] < 0 || ray_pose[i] >= U)
                return pg_fail(h, PG_EINVAL, "pg_poseopt_forward: ray_pose[%d] = %d is outside [0, %d)", i, ray_pose[i], U);
            ++seg_start[ray_pose[i] + 1];
        }
        for (int p = 0; p < U; ++p) seg_start[p + 1] += seg_start[p];
        std::vector<int32_t> fill(seg_start, seg_start + U);
        for (int i = 0; i < n; ++i) seg_rays[fill[ray_pose[i]]++] = i;
    }
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(upload(h, s, st));
    const int* d = s->d_idx.as<const int>();
    hipLaunchKernelGGL(poseopt_fwd_kernel, dim3((unsigned)U), dim3(THREADS), 0, st, bones, pelvis, rest_pose, (int)rest_stride, d, max_depth,
                       ray_pose ? d + TREE_WORDS : nullptr, ray_pose ? d + TREE_WORDS + U + 1 : nullptr, rots, l2ws, skts, kps);
    PG_LAUNCH_CHECK(h, "pose layer forward kernel");
    return PG_OK;
}

int pg_poseopt_backward(pg_handle* h, void* stream, int64_t n_poses, int rot_dim, const float* bones, const float* pelvis,
                        const float* rest_pose, int64_t rest_stride, const int32_t* parents, int64_t n_rays, const int32_t* seg_start,
                        const int32_t* seg_rays, const float* d_rots, const float* d_l2ws, const float* d_skts, const float* d_kps,
                        float* d_bones, float* d_pelvis) {
    using namespace pgp;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    State* s = nullptr;
    PG_TRY(pg_state(h, s));
    int max_depth = 0;
    PG_TRY(check_common(h, "pg_poseopt_backward", n_poses, rot_dim, bones, pelvis, rest_pose, rest_stride, parents, n_rays, s->host, &max_depth));
    if (!seg_start || (n_rays > 0 && !seg_rays) || !d_bones || !d_pelvis) return pg_fail(h, PG_EINVAL, "pg_poseopt_backward: null argument");
    const int U = (int)n_poses, n = (int)n_rays;
    // segments: monotone from 0 to n; every ray in exactly one of them; ascending inside a segment (the order of the sums)
    if (seg_start[0] != 0 || seg_start[U] != n)
        return pg_fail(h, PG_EINVAL, "pg_poseopt_backward: seg_start must run from 0 to n_rays (%d), got %d .. %d", n, seg_start[0], seg_start[U]);
    for (int p = 0; p < U; ++p)
        if (seg_start[p + 1] < seg_start[p] || seg_start[p + 1] > n)
            return pg_fail(h, PG_EINVAL, "pg_poseopt_backward: seg_start is not monotone at pose %d (%d, %d)", p, seg_start[p], seg_start[p + 1]);
    {
        std::vector<char> seen((size_t)n, 0);
        for (int p = 0; p < U; ++p)
            for (int i = seg_start[p]; i < seg_start[p + 1]; ++i) {
                const int r = seg_rays[i];
                if (r < 0 || r >= n || seen[r]) return pg_fail(h, PG_EINVAL, "pg_poseopt_backward: seg_rays is not a permutation of 0..%d (entry %d = %d)", n - 1, i, r);
                if (i > seg_start[p] && seg_rays[i - 1] >= r)
                    return pg_fail(h, PG_EINVAL, "pg_poseopt_backward: the rays of pose %d are not in ascending order (entry %d)", p, i);
                seen[r] = 1;
            }
    }
    if (U == 0) return PG_OK;
    int32_t* hs = s->host.data() + TREE_WORDS;
    for (int p = 0; p <= U; ++p) hs[p] = seg_start[p];
    for (int i = 0; i < n; ++i) hs[U + 1 + i] = seg_rays[i];
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(upload(h, s, st));
    const int* d = s->d_idx.as<const int>();
    hipLaunchKernelGGL(poseopt_bwd_kernel, dim3((unsigned)U), dim3(THREADS), 0, st, bones, pelvis, rest_pose, (int)rest_stride, d, max_depth,
                       d + TREE_WORDS, d + TREE_WORDS + U + 1, d_rots, d_l2ws, d_skts, d_kps, d_bones, d_pelvis);
    PG_LAUNCH_CHECK(h, "pose layer backward kernel");
    return PG_OK;
}

}  // extern "C"
