// pg_kin.h -- the 24-joint kinematic tree of the pose kernels, once: the chain product l2w_j = l2w_parent rel_j on rows 0..2 of a
// 4 x 4 and its transpose, the two rotation-vector maps with their transposes, the kps / l2ws / skts writer, and the host-side check
// of a `parents` table.  Used by pose_kinematics_kernel (pg_kernels.hip), the pose layer (pg_poseopt.hip), the key-point kinematics
// backward (pg_kploss.hip) and the SMPL body (pg_smpl.hip); DESIGN.md 2.12b.
// The library is built with -ffp-contract=on, which fuses within one statement: every statement below is the statement the kernels
// had, whole, and every sum keeps its order, so a kernel's doubles do not depend on which of these it calls.  Do not tidy them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgkin {

constexpr int NJ = 24;

// the joint tree as the kernels take it, by value: parent[root] = -1; level = distance from the root, depth the largest
struct KinTree { int parent[NJ], level[NJ], depth; };

// the constants of the key-point kinematics: offs[j] = rest[j] - rest[parent[j]] (rest[0] for the root)
struct KinConst { double offs[NJ * 3]; KinTree tree; };

// Fills kt from a parents table; false unless every joint after the root follows its parent (*bad: the first that does not).  The
// root's own entry is the caller's rule (0, -1 or either): it is not read, and parent[0] is stored as -1.
inline bool pg_kin_tree(const int32_t* parents, KinTree& kt, int* bad = nullptr) {
    kt.parent[0] = -1; kt.level[0] = 0; kt.depth = 0;
    for (int j = 1; j < NJ; ++j) {
        if (parents[j] < 0 || parents[j] >= j) {
            if (bad) *bad = j;
            return false;
        }
        kt.parent[j] = parents[j];
        kt.level[j] = kt.level[parents[j]] + 1;
        if (kt.level[j] > kt.depth) kt.depth = kt.level[j];
    }
    return true;
}

// the sum over the wave's 64 lanes, the same bits in every lane (a + b and b + a are the same number)
__device__ __forceinline__ double wave_all_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// out = P L on rows 0..2 of two 4 x 4 whose row 3 is 0 0 0 1 (out is neither P nor L)
__device__ __forceinline__ void mul34(const double* P, const double* L, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a0 = P[4 * r], a1 = P[4 * r + 1], a2 = P[4 * r + 2], a3 = P[4 * r + 3];
#pragma unroll
        for (int c = 0; c < 4; ++c) out[4 * r + c] = a0 * L[c] + a1 * L[4 + c] + a2 * L[8 + c] + (c == 3 ? a3 : 0.0);
    }
}

// The chain level by level on one pose's rows in LDS: joint j leaves its relative transform R in rel[j], and l2w[j] = l2w[par] R
// once its parent's level is done.  Called by every thread of the workgroup (barriers inside); `active`: the thread owns joint j.
__device__ __forceinline__ void chain_forward(double (*rel)[12], double (*l2w)[12], const double R[12], int j, bool active, int par, int lev,
                                              int depth) {
    if (active) {
#pragma unroll
        for (int e = 0; e < 12; ++e) rel[j][e] = R[e];
        if (lev == 0) {
#pragma unroll
            for (int e = 0; e < 12; ++e) l2w[j][e] = R[e];
        }
    }
    __syncthreads();
    for (int d = 1; d <= depth; ++d) {
        if (active && lev == d) mul34(l2w[par], R, l2w[j]);
        __syncthreads();
    }
}

// The second forward form, for a kernel that keeps one set of rows: the lane's joint-to-parent transform G becomes joint-to-world.
// Every lane leaves its own in the wave's LDS rows, then walks up its ancestors, `depth` steps for every lane (a lane that has
// reached the root keeps what it has).  The same products in the same order as chain_forward.
__device__ __forceinline__ void chain_to_world(double (*srel)[12], const int* spar, int j, bool jl, int depth, double G[12]) {
    if (jl) {
#pragma unroll
        for (int e = 0; e < 12; ++e) srel[j][e] = G[e];
    }
    __syncthreads();
    int p = spar[j];
    for (int s = 0; s < depth; ++s) {
        if (p >= 0) {
            double P[12], N[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = srel[p][e];
            mul34(P, G, N);
#pragma unroll
            for (int e = 0; e < 12; ++e) G[e] = N[e];
            p = spar[p];
        }
    }
}

// The chain backwards on the cotangents G of the l2w rows, children before parents: l2w_c = l2w_p rel_c gives G_p += G_c rel_c^T
// (rows 0..2; row 3 of rel_c is 0 0 0 1).  A parent starts from its own value and adds its children c > j in ascending joint order,
// each g0 L0 + g1 L1 + g2 L2 + g3 L3, in a register accumulator.  spar: the parents in LDS.  Barriers inside, as chain_forward.
__device__ __forceinline__ void chain_backward(double (*G)[12], const double (*rel)[12], const int* spar, int j, bool active, int lev, int depth) {
    for (int d = depth; d >= 1; --d) {
        if (active && lev == d - 1) {
            double acc[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) acc[e] = G[j][e];
            for (int c = j + 1; c < NJ; ++c) {
                if (spar[c] != j) continue;
                const double* g = G[c];
                const double* L = rel[c];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double g0 = g[4 * r], g1 = g[4 * r + 1], g2 = g[4 * r + 2], g3 = g[4 * r + 3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[4 * r + k] += g0 * L[4 * k] + g1 * L[4 * k + 1] + g2 * L[4 * k + 2] + g3 * L[4 * k + 3];
                    acc[4 * r + 3] += g3;
                }
            }
#pragma unroll
            for (int e = 0; e < 12; ++e) G[j][e] = acc[e];
        }
        __syncthreads();
    }
}

// The cotangent of rel_j from that of l2w_j: D = (l2w_parent^T G_j), its first C columns (3: the rotation; 4: with the translation),
// row-major with row stride C.  The root (par < 0) has the identity for a parent.
template <int C>
__device__ __forceinline__ void parent_transpose(const double (*l2w)[12], int par, const double* g, double* D) {
    if (par < 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) D[C * k + c] = g[4 * k + c];
    } else {
        const double* P = l2w[par];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) D[C * k + c] = P[k] * g[c] + P[4 + k] * g[4 + c] + P[8 + k] * g[8 + c];
    }
}

// a float32 rotation matrix, used as given, into rows 0..2 of [R | .]
__device__ __forceinline__ void rotmat_to_rows(const float* __restrict__ rp, double rel[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) rel[4 * r + c] = (double)rp[3 * r + c];
}

// what rotvec_to_rows leaves for its transpose: the unit quaternion, the vector, and the factors of dq -> dr
struct Quat {
    double r[3], q[4];       // q = x y z w, normalised
    double k, nrm, A, Bw;    // q_xyz = r k / nrm;  dk/dr_i = A r_i;  dq_w/dr_i = Bw r_i (before the normalisation)
};

// scipy's rotation vector -> unit quaternion -> matrix map: rows 0..2 of [R | .] into rel[0..2][0..2].  Below theta = 1e-3 the
// series in theta^2 (k = 1/2 - t/48 + t^2/3840), finite at zero.
__device__ __forceinline__ void rotvec_to_rows(const double* __restrict__ b, Quat& s, double rel[12]) {
    s.r[0] = b[0]; s.r[1] = b[1]; s.r[2] = b[2];
    const double t2 = s.r[0] * s.r[0] + s.r[1] * s.r[1] + s.r[2] * s.r[2], th = sqrt(t2);
    const bool small = th < 1e-3;
    double qw;
    if (small) {
        s.k = 0.5 - t2 / 48.0 + t2 * t2 / 3840.0;
        s.A = 2.0 * (-1.0 / 48.0 + t2 / 1920.0);
        s.Bw = 2.0 * (-1.0 / 8.0 + t2 / 192.0);
        qw = cos(0.5 * th);                                 // (the series 1 - t/8 + t^2/384 to below 1e-22: the forward's value)
    } else {
        const double sh = sin(0.5 * th);
        qw = cos(0.5 * th);
        s.k = sh / th;
        s.A = (0.5 * qw * th - sh) / (t2 * th);             // k'(theta) / theta
        s.Bw = -0.5 * s.k;
    }
    double qx = s.r[0] * s.k, qy = s.r[1] * s.k, qz = s.r[2] * s.k;
    s.nrm = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= s.nrm; qy /= s.nrm; qz /= s.nrm; qw /= s.nrm;
    s.q[0] = qx; s.q[1] = qy; s.q[2] = qz; s.q[3] = qw;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, ww = qw * qw;
    const double xy = qx * qy, zw = qz * qw, xz = qx * qz, yw = qy * qw, yz = qy * qz, xw = qx * qw;
    rel[0] = xx - yy - zz + ww; rel[1] = 2.0 * (xy - zw);    rel[2] = 2.0 * (xz + yw);
    rel[4] = 2.0 * (xy + zw);   rel[5] = -xx + yy - zz + ww; rel[6] = 2.0 * (yz - xw);
    rel[8] = 2.0 * (xz - yw);   rel[9] = 2.0 * (yz + xw);    rel[10] = -xx - yy + zz + ww;
}

// the transpose of rotvec_to_rows: D = the cotangent of R (row-major 3 x 3) -> the cotangent of the rotation vector
__device__ __forceinline__ void rotvec_bwd(const Quat& s, const double D[9], double o[3]) {
    const double x = s.q[0], y = s.q[1], z = s.q[2], w = s.q[3];
    const double s01 = D[1] + D[3], s02 = D[2] + D[6], s12 = D[5] + D[7];
    const double a21 = D[7] - D[5], a02 = D[2] - D[6], a10 = D[3] - D[1];
    double dq[4];
    dq[0] = 2.0 * (x * (D[0] - D[4] - D[8]) + y * s01 + z * s02 + w * a21);
    dq[1] = 2.0 * (y * (-D[0] + D[4] - D[8]) + x * s01 + z * s12 + w * a02);
    dq[2] = 2.0 * (z * (-D[0] - D[4] + D[8]) + x * s02 + y * s12 + w * a10);
    dq[3] = 2.0 * (w * (D[0] + D[4] + D[8]) + x * a21 + y * a02 + z * a10);
    // q = u / |u|
    const double t = x * dq[0] + y * dq[1] + z * dq[2] + w * dq[3];
    double du[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) du[i] = (dq[i] - s.q[i] * t) / s.nrm;
    // u_xyz = r k(theta), u_w = c(theta)
    const double dr = du[0] * s.r[0] + du[1] * s.r[1] + du[2] * s.r[2];
    const double f = s.A * dr + s.Bw * du[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = s.k * du[i] + s.r[i] * f;
}

// what rodrigues_as_written leaves for its transpose
struct Rodrigues {
    double rv[3], angle, sn, cs, Km[9];
};

// batch_rodrigues (smplx lbs.py:295-329) as written: angle = |r + 1e-8|, rot_dir = r / angle, R = I + sin K + (1 - cos) K K, into
// rows 0..2 of [R | .]
__device__ __forceinline__ void rodrigues_as_written(const float* __restrict__ rp, Rodrigues& s, double rel[12]) {
    s.rv[0] = (double)rp[0]; s.rv[1] = (double)rp[1]; s.rv[2] = (double)rp[2];
    const double e0 = s.rv[0] + 1e-8, e1 = s.rv[1] + 1e-8, e2 = s.rv[2] + 1e-8;
    s.angle = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    const double x = s.rv[0] / s.angle, y = s.rv[1] / s.angle, z = s.rv[2] / s.angle;
    s.sn = sin(s.angle); s.cs = cos(s.angle);
    const double Km[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double kk = Km[3 * r] * Km[c] + Km[3 * r + 1] * Km[3 + c] + Km[3 * r + 2] * Km[6 + c];
            rel[4 * r + c] = (r == c ? 1.0 : 0.0) + s.sn * Km[3 * r + c] + (1.0 - s.cs) * kk;
            s.Km[3 * r + c] = Km[3 * r + c];
        }
}

// the transpose of rodrigues_as_written: dR = the cotangent of R (row-major 3 x 3) -> the cotangent of the three numbers
__device__ __forceinline__ void rodrigues_as_written_bwd(const Rodrigues& s, const double dR[9], double o[3]) {
    const double* Km = s.Km;
    const double sn = s.sn, cs = s.cs, angle = s.angle;
    const double oc = 1.0 - cs;
    double dK[9], dth = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // (D K^T + K^T D)[r][c] = sum_k D[r][k] K[c][k] + K[k][r] D[k][c]
            double t = 0.0, kk = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t += dR[3 * r + k] * Km[3 * c + k] + Km[3 * k + r] * dR[3 * k + c];
                kk += Km[3 * r + k] * Km[3 * k + c];
            }
            dK[3 * r + c] = sn * dR[3 * r + c] + oc * t;
            dth += dR[3 * r + c] * (cs * Km[3 * r + c] + sn * kk);
        }
    const double dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    dth -= (dd[0] * s.rv[0] + dd[1] * s.rv[1] + dd[2] * s.rv[2]) / (angle * angle);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = dd[c] / angle + dth * (s.rv[c] + 1e-8) / angle;
}

// One joint's rows G of l2w to the outputs that were asked for, at joint index `at` (pose * 24 + joint): kps = column 3, l2ws the
// 4 x 4 in double, skts its rigid inverse [R^T | -R^T t]; float32 outputs rounded once.
__device__ __forceinline__ void write_pose_outputs(const double* G, size_t at, float* __restrict__ kps, double* __restrict__ l2ws,
                                                   float* __restrict__ skts) {
    if (kps) { kps[at * 3] = (float)G[3]; kps[at * 3 + 1] = (float)G[7]; kps[at * 3 + 2] = (float)G[11]; }
    if (l2ws) {
        double* o = l2ws + at * 16;
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = G[e];
        o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
    }
    if (skts) {
        float* o = skts + at * 16;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            o[4 * r] = (float)G[r]; o[4 * r + 1] = (float)G[4 + r]; o[4 * r + 2] = (float)G[8 + r];
            o[4 * r + 3] = (float)(-(G[r] * G[3] + G[4 + r] * G[7] + G[8 + r] * G[11]));
        }
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    }
}

}  // namespace pgkin
