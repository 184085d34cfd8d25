// pg_posescore.hip -- 3-D poses scored against their ground truth on the device: MPJPE, and the MPJPE after one of
// three alignments of the prediction -- the least-squares scale of Criterion3DPose_leastQuaresScaled
// (core/utils/evaluation_helpers.py:506-522), the Procrustes fit of `procrustes(scaling=True, reflection='best')` (:387-467) and the
// det(R) = +1 fit of compute_similarity_transform (run_gan.py:1380-1428) -- with the shares of joint distances below a list of
// thresholds (PCK; :595-601).
//   pose_scores_kernel     : one wave per pose, lane j owns joint j (J <= 64).  The lane widens its joint of both sets to double; means,
//                            norms and the nine cross-covariance entries are xor-butterflies over all 64 lanes (lanes >= J add
//                            zeros), so every lane ends with the same bits and runs the 3 x 3 part (pg_pose_align.h) uniformly.
//                            A wave walks the poses w, w + n_waves, ...: the per-pose values go to per_pose / aligned / joint_err,
//                            their sums and the threshold counts (lane t counts threshold t) stay in registers and go to the
//                            wave's slot at the end.
//   pose_scores_sum_kernel : the slots folded in a fixed order into summary[4 + 2 T]; one workgroup.
// No atomics; every sum has a fixed order for a given B, and a pose's own numbers do not depend on the batch around it.  No loop
// depends on a value of the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_handle.h"
#include "pg_kin.h"
#include "pg_pose_align.h"

namespace pgq {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_BLOCKS = 1024;
constexpr int MAXJ = 64, MAXT = 64;
constexpr int SLOT_SUMS = 4;                 // raw, aligned, d, unused: 32 bytes
// a wave's slot: SLOT_SUMS doubles, then 2 * MAXT 32-bit counts (raw, aligned)
constexpr size_t SLOT_BYTES = SLOT_SUMS * sizeof(double) + 2 * MAXT * sizeof(uint32_t);

struct Args {
    const float* pred;
    const float* gt;
    long long B;
    int J_in, J, root, align, T;
    int has_joints;
    double* per_pose;
    float* aligned;
    float* joint_err;
    uint8_t* slots;
    int32_t joints[MAXJ];
    double thr[MAXT];
};

using pgkin::wave_all_sum;
__global__ __launch_bounds__(THREADS) void pose_scores_kernel(Args a) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * WAVES;
    const int J = a.J;
    const bool live = lane < J;
    // the lane's row of J_in (lanes >= J: row 0, never read)
    int row = live ? lane : 0;
    if (a.has_joints && live) row = a.joints[lane];
    const double inv_j = 1.0 / (double)J;

    double sum_raw = 0.0, sum_al = 0.0, sum_d = 0.0;
    uint32_t cnt_raw = 0, cnt_al = 0;                      // lane t: joint distances below thr[t] so far

    // every lane of the wave takes every trip: the shuffles below need all 64
    for (long long pose = wave; pose < a.B; pose += n_waves) {
        const float* pp = a.pred + ((size_t)pose * a.J_in) * 3;
        const float* gp = a.gt + ((size_t)pose * a.J_in) * 3;
        double p[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        if (live) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { p[c] = (double)pp[(size_t)row * 3 + c]; g[c] = (double)gp[(size_t)row * 3 + c]; }
        }
        double poison = 0.0;                               // 0, or NaN for a pose with a non-finite coordinate
        if (a.root >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double pr = (double)pp[(size_t)a.root * 3 + c], gr = (double)gp[(size_t)a.root * 3 + c];
                poison += 0.0 * pr + 0.0 * gr;
                if (live) { p[c] -= pr; g[c] -= gr; }
            }
        }
        poison += 0.0 * (p[0] + p[1] + p[2]) + 0.0 * (g[0] + g[1] + g[2]);
        poison = wave_all_sum(poison);

        // the joint's distance as it is
        const double dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
        const double dist_raw = sqrt(dx * dx + dy * dy + dz * dz) + poison;
        const double raw = wave_all_sum(live ? dist_raw : 0.0) * inv_j;

        // means and centred sets (X = g the target, Y = p the set that moves)
        double mx[3], x0[3], y0[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mx[c] = wave_all_sum(g[c]) * inv_j;
            const double my = wave_all_sum(p[c]) * inv_j;
            x0[c] = live ? g[c] - mx[c] : 0.0;
            y0[c] = live ? p[c] - my : 0.0;
        }
        const double ssx = wave_all_sum(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);

        double z[3], scale;
        if (a.align == PG_POSE_ALIGN_NONE) {
            z[0] = p[0]; z[1] = p[1]; z[2] = p[2];
            scale = 1.0;
        } else if (a.align == PG_POSE_ALIGN_SCALE) {
            const double pg_ = wave_all_sum(p[0] * g[0] + p[1] * g[1] + p[2] * g[2]);
            const double pp_ = wave_all_sum(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
            scale = pg_ / pp_;
            z[0] = scale * p[0]; z[1] = scale * p[1]; z[2] = scale * p[2];
        } else {
            const double ssy = wave_all_sum(y0[0] * y0[0] + y0[1] * y0[1] + y0[2] * y0[2]);
            const double nx = sqrt(ssx), ny = sqrt(ssy);
            double xn[3], yn[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { xn[c] = x0[c] / nx; yn[c] = y0[c] / ny; }        // 0 / 0 = NaN for a set without spread
            double A[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) A[3 * r + c] = wave_all_sum(live ? xn[r] * yn[c] : 0.0);
            const pgalign::Result f = pgalign::align(A, a.align == PG_POSE_ALIGN_ROTATION);
            const double k = nx * f.sum_s;
#pragma unroll
            for (int c = 0; c < 3; ++c) z[c] = k * (yn[0] * f.T[c] + yn[1] * f.T[3 + c] + yn[2] * f.T[6 + c]) + mx[c];
            scale = f.sum_s * nx / ny;
        }
        const double ex = z[0] - g[0], ey = z[1] - g[1], ez = z[2] - g[2];
        const double sq = ex * ex + ey * ey + ez * ez;
        const double dist_al = sqrt(sq) + poison;
        const double al = wave_all_sum(live ? dist_al : 0.0) * inv_j;
        const double d = wave_all_sum(live ? sq : 0.0) / ssx + poison;
        scale += poison;

        if (live) {
            if (a.aligned) {
                float* o = a.aligned + ((size_t)pose * J + lane) * 3;
                o[0] = (float)(z[0] + poison); o[1] = (float)(z[1] + poison); o[2] = (float)(z[2] + poison);
            }
            if (a.joint_err) a.joint_err[(size_t)pose * J + lane] = (float)dist_al;
        }
        if (a.per_pose && lane < 4)
            a.per_pose[(size_t)pose * 4 + lane] = lane == 0 ? raw : lane == 1 ? al : lane == 2 ? d : scale;
        sum_raw += raw; sum_al += al; sum_d += d;

        // lane t counts threshold t: a ballot per threshold (a NaN distance is below nothing)
        for (int t = 0; t < a.T; ++t) {
            const double th = a.thr[t];
            const uint32_t nr = (uint32_t)__popcll(__ballot(live && dist_raw < th));
            const uint32_t na = (uint32_t)__popcll(__ballot(live && dist_al < th));
            if (lane == t) { cnt_raw += nr; cnt_al += na; }
        }
    }

    uint8_t* slot = a.slots + (size_t)wave * SLOT_BYTES;
    if (lane < SLOT_SUMS) reinterpret_cast<double*>(slot)[lane] = lane == 0 ? sum_raw : lane == 1 ? sum_al : lane == 2 ? sum_d : 0.0;
    uint32_t* cs = reinterpret_cast<uint32_t*>(slot + SLOT_SUMS * sizeof(double));
    cs[lane] = cnt_raw;
    cs[MAXT + lane] = cnt_al;
}

// summary = B, the three means, the 2 T shares.  Wave q < 3: lane l adds sum q of slots l, l + 64, ... in that order, then the
// butterfly; threads 0 .. 2 T - 1 of the workgroup each add one count over the slots in index order.
__global__ __launch_bounds__(THREADS) void pose_scores_sum_kernel(const uint8_t* __restrict__ slots, int n_slots, long long B, int J, int T,
                                                                 double* __restrict__ summary) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (wv < 3) {
        double acc = 0.0;
        for (int s = lane; s < n_slots; s += 64) acc += reinterpret_cast<const double*>(slots + (size_t)s * SLOT_BYTES)[wv];
        acc = wave_all_sum(acc);
        if (lane == 0) summary[1 + wv] = acc / (double)B;
    }
    if (tid == THREADS - 1) summary[0] = (double)B;
    if (tid < 2 * T) {
        const int which = tid / T, t = tid - which * T;
        unsigned long long n = 0;
        for (int s = 0; s < n_slots; ++s)
            n += reinterpret_cast<const uint32_t*>(slots + (size_t)s * SLOT_BYTES + SLOT_SUMS * sizeof(double))[which * MAXT + t];
        summary[4 + tid] = (double)n / ((double)B * (double)J);
    }
}

}  // namespace pgq

// ---- the host side --------------------------------------------------------------------------------------------------------------------
namespace {

// the waves' slots.  One buffer per handle: calls on one handle are serialised by the caller (as pg_metrics.hip).
struct PoseScoreState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_POSESCORE;
    ~PoseScoreState() override { pg_release(slots); }
    DevBuf slots;
};
static_assert(pgq::MAXJ == PG_POSE_MAX_JOINTS, "pg_check_joint_selection bounds J for the kernel's joint table");

}  // namespace

extern "C" int pg_pose_scores(pg_handle* h, void* stream, int64_t B, int J_in, const float* pred, const float* gt, const int32_t* joints, int J,
                              int root, int align, const double* thresholds, int T, double* per_pose, float* aligned, float* joint_err,
                              double* summary) {
    const char* who = "pg_pose_scores";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!pred || !gt || !summary) return pg_fail(h, PG_EINVAL, "%s: pred, gt and summary are required", who);
    if (B < 1) return pg_fail(h, PG_EINVAL, "%s: B = %lld", who, (long long)B);
    PG_TRY(pg_check_joint_selection(h, who, J_in, joints, &J, root, false));
    if (align < PG_POSE_ALIGN_NONE || align > PG_POSE_ALIGN_ROTATION) return pg_fail(h, PG_EINVAL, "%s: unknown alignment mode %d", who, align);
    if (T < 0 || T > pgq::MAXT) return pg_fail(h, PG_EINVAL, "%s: T = %d is outside [0, %d]", who, T, pgq::MAXT);
    if (T > 0 && !thresholds) return pg_fail(h, PG_EINVAL, "%s: T = %d without thresholds", who, T);
    if (pg_misaligned(pred, sizeof(float)) || pg_misaligned(gt, sizeof(float)) || pg_misaligned(aligned, sizeof(float)) ||
        pg_misaligned(joint_err, sizeof(float)) || pg_misaligned(per_pose, sizeof(double)) || pg_misaligned(summary, sizeof(double)))
        return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);

    PoseScoreState* s = nullptr;
    PG_TRY(pg_state(h, s));
    const long long want = (B + pgq::WAVES - 1) / pgq::WAVES;
    const int blocks = (int)(want < pgq::MAX_BLOCKS ? want : pgq::MAX_BLOCKS);
    const int n_slots = blocks * pgq::WAVES;
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(pg_grow(h, s->slots, (size_t)n_slots * pgq::SLOT_BYTES, "pose score slots", (size_t)pgq::MAX_BLOCKS * pgq::WAVES * pgq::SLOT_BYTES));

    pgq::Args a{};
    a.pred = pred; a.gt = gt; a.B = B; a.J_in = J_in; a.J = J; a.root = root; a.align = align; a.T = T;
    a.has_joints = joints ? 1 : 0;
    a.per_pose = per_pose; a.aligned = aligned; a.joint_err = joint_err; a.slots = s->slots.as<uint8_t>();
    for (int j = 0; j < J; ++j) a.joints[j] = joints ? joints[j] : j;
    for (int t = 0; t < T; ++t) a.thr[t] = thresholds[t];
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pgq::pose_scores_kernel, dim3((unsigned)blocks), dim3(pgq::THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "pose scores kernel");
    hipLaunchKernelGGL(pgq::pose_scores_sum_kernel, dim3(1), dim3(pgq::THREADS), 0, st, s->slots.as<const uint8_t>(), n_slots, (long long)B, J, T,
                       summary);
    PG_LAUNCH_CHECK(h, "pose scores sum kernel");
    return PG_OK;
}
