// pg_trainloss.hip -- what an A-NeRF training step optimises: the reference Trainer's losses, pose regulariser and
// gradient norms (core/trainer.py:193-205, 321-443), each with its gradients in the same call.
//   loss_part_kernel   : one ray per thread, 256 rays per workgroup.  Both passes' composite on the background, loss element (MSE / L1 /
//                        smooth-L1), squared error for PSNR, masked BCE term and count, and acc_map for the `alpha` stat; the
//                        workgroup's nine sums in a fixed tree -> part[block][9].
//   loss_grad_kernel   : every workgroup folds the BCE counts out of `part` again (thread t adds blocks t, t + 256, ... in that order,
//                        then the tree: the same bits in every workgroup), writes its 256 rays' gradients; workgroup 0 also folds the
//                        other seven columns and writes the summary.
//   reg_kernel         : _compute_kp_loss for opt_rot6d: one (ray, joint) per thread.  The gradients do not depend on any sum (the
//                        means' denominators are n 23 and n 24), so d_rots / d_kps are written here with the workgroup's three
//                        partial sums; reg_final_kernel (one workgroup) folds them into the summary.
//   norm_part_kernel   : get_gradnorm: one workgroup per 16384-element segment of a tensor.  Element i of a tensor always lands in
//                        slot i mod 1024, whatever the pointer's alignment: the aligned 16-byte loads start `m` elements in front
//                        of the segment (m = 0..3), head and tail quads are read element by element, and thread t's four
//                        accumulators are slots (4 t + c - m) mod 1024.  The 1024 slots fold in a fixed tree -> part[block].
//   norm_final_kernel  : thread t adds tensor t's segments in ascending order -> its norm; the squares fold in a tree -> total, avg.
// float64 arithmetic, outputs rounded once; no atomics; the split into partial sums depends on the sizes alone (not on the device,
// not on where a tensor lies); nothing is kept between calls except grow-only scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "pg_handle.h"
#include "pg_sumsq.h"

namespace pgtl {

constexpr int NJ = 24;
constexpr int THREADS = pgsq::THREADS;
constexpr int NQ = 9;             // loss_part_kernel's columns: pass p at 4 p + (0 loss, 1 squared error, 2 BCE sum, 3 BCE count); 8 = sum of acc_map
constexpr int RQ = 3;             // reg_kernel's columns: kp, temporal, per-joint change
constexpr int SEG = pgsq::SEG;    // elements of one norm_part_kernel workgroup
constexpr int SLOTS = pgsq::SLOTS;
constexpr double BCE_EPS = 1e-8;  // acc2bce's eps (trainer.py:44)

// the sum of the workgroup's 256 values in a fixed tree, the same bits in every thread
__device__ __forceinline__ double block_sum(double v, double* lds) {
    const int tid = threadIdx.x;
    __syncthreads();                                         // (the last call's readers are done with lds[0])
    lds[tid] = v;
    __syncthreads();
    for (int d = THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) lds[tid] += lds[tid + d];
        __syncthreads();
    }
    return lds[0];
}

// column q of part[nblocks][stride]: thread t adds rows t, t + 256, ... in that order, then the tree
__device__ __forceinline__ double column_sum(const double* __restrict__ part, long long nblocks, int stride, int q, double* lds) {
    double acc = 0.0;
    for (long long b = threadIdx.x; b < nblocks; b += THREADS) acc += part[b * stride + q];
    return block_sum(acc, lds);
}

// ---- the photometric loss -----------------------------------------------------------------------------------------------------------
struct LossArgs {
    const float* rgb[2];
    const float* acc[2];
    const float* target;
    const float* bgs;
    const float* fgs;
    long long n, nblocks;
    int n_pass, loss_kind, use_bg, reg_kind;
    double beta, base_bg, coarse_weight, reg_coef;
    double* part;
    double* summary;
    float* d_rgb[2];
    float* d_acc[2];
};

__device__ __forceinline__ double loss_elem(int kind, double beta, double d) {
    const double ad = fabs(d);
    if (kind == PG_TRAIN_LOSS_MSE) return d * d;
    if (kind == PG_TRAIN_LOSS_L1) return ad;
    return ad < beta ? 0.5 * d * d / beta : ad - 0.5 * beta;             // F.smooth_l1_loss; NaN takes the linear branch and stays NaN
}

__device__ __forceinline__ double loss_elem_grad(int kind, double beta, double d) {
    if (kind == PG_TRAIN_LOSS_MSE) return 2.0 * d;
    if (kind == PG_TRAIN_LOSS_HUBER && fabs(d) < beta) return d / beta;
    return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d);                         // sign(d): 0 at 0 as in torch, NaN stays
}

// one ray of one pass: the composited prediction minus the target, and the background the acc gradient needs
__device__ __forceinline__ void ray_diff(const LossArgs& a, int p, long long i, double d[3], double bg[3], double& x) {
    x = (double)a.acc[p][i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        bg[c] = a.bgs ? (double)a.bgs[i * 3 + c] : a.base_bg;
        double pred = (double)a.rgb[p][i * 3 + c];
        if (a.use_bg) pred = pred + (1.0 - x) * bg[c];
        d[c] = pred - (double)a.target[i * 3 + c];
    }
}

__global__ __launch_bounds__(THREADS) void loss_part_kernel(LossArgs a) {
    __shared__ double lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    double v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = 0.0;
    if (i < a.n) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (p >= a.n_pass) break;
            double d[3], bg[3], x;
            ray_diff(a, p, i, d, bg, x);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[4 * p] += loss_elem(a.loss_kind, a.beta, d[c]);
                v[4 * p + 1] += d[c] * d[c];
            }
            if (a.reg_kind == PG_TRAIN_REG_BCE) {
                const double y = (double)a.fgs[i];
                if (y < 1.0) {                                           // acc2bce(reduction='off'): the rays with y < 1.0 only
                    v[4 * p + 2] = -(y * log(x + BCE_EPS) + (1.0 - y) * log(1.0 - x + BCE_EPS));
                    v[4 * p + 3] = 1.0;
                }
            }
            if (p == 0) v[8] = x;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double s = block_sum(v[q], lds);
        if (threadIdx.x == 0) a.part[(long long)blockIdx.x * NQ + q] = s;
    }
}

__global__ __launch_bounds__(THREADS) void loss_grad_kernel(LossArgs a, int with_grads) {
    __shared__ double lds[THREADS];
    double cnt[2] = {0.0, 0.0};
    if (a.reg_kind == PG_TRAIN_REG_BCE) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (p < a.n_pass) cnt[p] = column_sum(a.part, a.nblocks, NQ, 4 * p + 3, lds);
    }
    const double n3 = 3.0 * (double)a.n;
    if (blockIdx.x == 0) {
        double s[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] = column_sum(a.part, a.nblocks, NQ, q, lds);
        if (threadIdx.x == 0) {
            const double ln10 = log(10.0);
            double loss[2] = {0.0, 0.0}, reg[2] = {0.0, 0.0}, psnr[2] = {0.0, 0.0};
            double total = 0.0;                                          // compute_loss's order: rgb_loss, reg_loss, rgb_loss0, reg_loss0
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (p >= a.n_pass) break;
                loss[p] = s[4 * p] / n3;
                if (p == 1) loss[p] = loss[p] * a.coarse_weight;
                psnr[p] = -10.0 * log(s[4 * p + 1] / n3) / ln10;
                total += loss[p];
                if (a.reg_kind == PG_TRAIN_REG_BCE) {
                    reg[p] = s[4 * p + 2] / s[4 * p + 3] * a.reg_coef;   // no ray with y < 1: 0 / 0, torch.mean of an empty tensor
                    total += reg[p];
                }
            }
            a.summary[0] = total;
            a.summary[1] = loss[0]; a.summary[2] = loss[1];
            a.summary[3] = reg[0];  a.summary[4] = reg[1];
            a.summary[5] = psnr[0]; a.summary[6] = psnr[1];
            a.summary[7] = s[8] / (double)a.n;
            a.summary[8] = s[3];    a.summary[9] = s[7];
        }
    }
    if (!with_grads) return;
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.n) return;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p >= a.n_pass) break;
        double d[3], bg[3], x;
        ray_diff(a, p, i, d, bg, x);
        const double w = (p == 1 ? a.coarse_weight : 1.0) / n3;
        double da = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double g = w * loss_elem_grad(a.loss_kind, a.beta, d[c]);
            if (a.d_rgb[p]) a.d_rgb[p][i * 3 + c] = (float)g;
            if (a.use_bg) da -= g * bg[c];
        }
        if (a.reg_kind == PG_TRAIN_REG_BCE && cnt[p] > 0.0) {
            const double y = (double)a.fgs[i];
            if (y < 1.0) da += a.reg_coef / cnt[p] * -(y / (x + BCE_EPS) - (1.0 - y) / (1.0 - x + BCE_EPS));
        }
        if (a.d_acc[p]) a.d_acc[p][i] = (float)da;
    }
}

// ---- the pose regulariser -----------------------------------------------------------------------------------------------------------
struct RegArgs {
    const float* rots;
    const float* kps;
    const float* a_rots;
    const float* a_kps;
    const int32_t* kp_idx;       // device copy of the caller's host array, every entry checked
    const float* p_rots;
    const float* p_kps;
    const float* n_rots;
    const float* n_kps;
    const float* temp_val;
    long long n, nblocks;
    int temporal;
    double tol, coef, temp_coef, ext_scale;
    double* part;
    double* summary;
    float* d_rots;
    float* d_kps;
};

__global__ __launch_bounds__(THREADS) void reg_kernel(RegArgs a) {
    __shared__ double lds[THREADS];
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    double v[RQ] = {0.0, 0.0, 0.0};
    if (e < a.n * NJ) {
        const long long ray = e / NJ;
        const int j = (int)(e - ray * NJ);
        const long long ae = (long long)a.kp_idx[ray] * NJ + j;
        const double ck = a.coef / ((double)a.n * (NJ - 1)), ct = a.temp_coef / ((double)a.n * NJ);
        const double tv = a.temporal ? (double)a.temp_val[ray] : 0.0;
        double g[9], gk[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            g[3 * r + 2] = 0.0;                              // the 6-D bone is columns 0 and 1: [..., :3, :2].flatten(-2)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int k = 3 * r + c;
                const double b = (double)a.rots[e * 9 + k];
                double gb = 0.0;
                if (j >= 1) {                                // the root is left out of kp_loss
                    const double df = (double)a.a_rots[ae * 9 + k] - b, x = df * df;
                    if (x > a.tol) { v[0] += x - a.tol; gb = -2.0 * df * ck; }
                    else if (x != x) v[0] += x;             // (a NaN reaches the sum, as through the reference's lerp)
                }
                if (a.temporal) {
                    const double u = (b - (double)a.p_rots[e * 9 + k]) - ((double)a.n_rots[e * 9 + k] - b);
                    v[1] += u * u;
                    gb += 4.0 * u * ct * tv;
                }
                g[k] = gb;
            }
        }
        double dist = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double kp = (double)a.kps[e * 3 + c], df = (double)a.a_kps[ae * 3 + c] - kp;
            dist += df * df;
            gk[c] = 0.0;
            if (a.temporal) {
                const double u = (kp - (double)a.p_kps[e * 3 + c]) - ((double)a.n_kps[e * 3 + c] - kp);
                v[1] += u * u;
                gk[c] = 4.0 * u * ct * tv;
            }
        }
        v[1] *= tv;
        v[2] = sqrt(dist);
        if (a.d_rots) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.d_rots[e * 9 + k] = (float)g[k];
        }
        if (a.d_kps) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.d_kps[e * 3 + c] = (float)gk[c];
        }
    }
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
        const double s = block_sum(v[q], lds);
        if (threadIdx.x == 0) a.part[(long long)blockIdx.x * RQ + q] = s;
    }
}

// summary = kp_loss, temp_loss, MPJPC, kp_loss + temp_loss
__global__ __launch_bounds__(THREADS) void reg_final_kernel(RegArgs a) {
    __shared__ double lds[THREADS];
    double s[RQ];
#pragma unroll
    for (int q = 0; q < RQ; ++q) s[q] = column_sum(a.part, a.nblocks, RQ, q, lds);
    if (threadIdx.x == 0) {
        const double kp = s[0] / ((double)a.n * (NJ - 1)) * a.coef;
        const double tp = a.temporal ? s[1] / ((double)a.n * NJ) * a.temp_coef : 0.0;
        a.summary[0] = kp;
        a.summary[1] = tp;
        a.summary[2] = s[2] / ((double)a.n * NJ) / a.ext_scale;
        a.summary[3] = kp + tp;
    }
}

// ---- the gradient norms -------------------------------------------------------------------------------------------------------------
struct NormEntry {
    const float* p;
    long long count;
    long long first_block;       // the tensor's segments are workgroups first_block .. first_block + ceil(count / SEG) - 1
};

__global__ __launch_bounds__(THREADS) void norm_part_kernel(const NormEntry* __restrict__ tab, int n_tensors, double* __restrict__ part) {
    __shared__ double lds[SLOTS];
    __shared__ int s_t;
    const int tid = threadIdx.x;
    if (tid < n_tensors) {
        const long long fb = tab[tid].first_block, nb = (tab[tid].count + SEG - 1) / SEG;
        if ((long long)blockIdx.x >= fb && (long long)blockIdx.x < fb + nb) s_t = tid;       // (exactly one tensor owns a workgroup)
    }
    __syncthreads();
    const NormEntry en = tab[s_t];
    const long long seg = (long long)blockIdx.x - en.first_block;
    const float* base = en.p + seg * SEG;
    const long long rest = en.count - seg * SEG;
    const int len = rest < SEG ? (int)rest : SEG;
    const double sq = pgsq::segment_sumsq(base, len, lds);                // (pg_sumsq.h: shared with pg_adam_step's clipping norm)
    if (tid == 0) part[blockIdx.x] = sq;
}

// out = total_norm, avg_norm, then every tensor's norm
__global__ __launch_bounds__(THREADS) void norm_final_kernel(const NormEntry* __restrict__ tab, int n_tensors, const double* __restrict__ part,
                                                             double* __restrict__ out) {
    __shared__ double lds[THREADS];
    const int tid = threadIdx.x;
    double sq = 0.0;
    if (tid < n_tensors) {
        const long long fb = tab[tid].first_block, nb = (tab[tid].count + SEG - 1) / SEG;
        for (long long b = 0; b < nb; ++b) sq += part[fb + b];
        out[2 + tid] = sqrt(sq);
    }
    const double total = block_sum(sq, lds);
    if (tid == 0) {
        out[0] = sqrt(total);
        out[1] = sqrt(total / (double)n_tensors);
    }
}

// what the three entry points keep in the handle: their partial sums, the device copies of kp_idx and of the tensor table, and the
// host copies an upload reads while it is in flight (as pg_poseopt.hip).  Calls on one handle are serialised by the caller.
struct State : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_TRAINLOSS;
    ~State() override { for (DevBuf* b : {&loss_part, &reg_part, &norm_part, &d_idx, &d_tab}) pg_release(*b); }
    DevBuf loss_part, reg_part, norm_part;
    DevBuf d_idx, d_tab;
    std::vector<int32_t> host_idx;
    std::vector<NormEntry> host_tab;
};

}  // namespace pgtl

extern "C" int pg_train_loss(pg_handle* h, void* stream, int64_t n, const float* rgb_map, const float* acc_map, const float* rgb0,
                             const float* acc0, const float* target, const float* bgs, double base_bg, const float* fgs, int loss_kind,
                             double beta, int use_background, double coarse_weight, int reg_kind, double reg_coef, double* summary,
                             float* d_rgb_map, float* d_acc_map, float* d_rgb0, float* d_acc0) {
    using namespace pgtl;
    const char* who = "pg_train_loss";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!rgb_map || !acc_map || !target || !summary) return pg_fail(h, PG_EINVAL, "%s: rgb_map, acc_map, target and summary are required", who);
    if ((rgb0 == nullptr) != (acc0 == nullptr)) return pg_fail(h, PG_EINVAL, "%s: rgb0 and acc0 come together (both NULL: no coarse pass)", who);
    if (!rgb0 && (d_rgb0 || d_acc0)) return pg_fail(h, PG_EINVAL, "%s: d_rgb0 / d_acc0 without a coarse pass", who);
    if (n < 1 || n > 0x7fffffffll) return pg_fail(h, PG_EINVAL, "%s: n = %lld is outside [1, 2^31 - 1]", who, (long long)n);
    if (loss_kind != PG_TRAIN_LOSS_MSE && loss_kind != PG_TRAIN_LOSS_L1 && loss_kind != PG_TRAIN_LOSS_HUBER)
        return pg_fail(h, PG_EINVAL, "%s: unknown loss_kind %d", who, loss_kind);
    if (loss_kind == PG_TRAIN_LOSS_HUBER && !(beta >= 0.0)) return pg_fail(h, PG_EINVAL, "%s: beta = %g (smooth-L1 needs beta >= 0)", who, beta);
    if (reg_kind == PG_TRAIN_REG_L1 || reg_kind == PG_TRAIN_REG_MSE)
        return pg_fail(h, PG_EINVAL, "%s: reg_fn = L1 / MSE is refused: the reference calls it with reduction='off', which img2l1 / img2mse "
                       "do not know and answer with the unreduced [n] tensor, so its total_loss has shape [n] and backward() raises; "
                       "only BCE trains there", who);
    if (reg_kind != PG_TRAIN_REG_NONE && reg_kind != PG_TRAIN_REG_BCE) return pg_fail(h, PG_EINVAL, "%s: unknown reg_kind %d", who, reg_kind);
    if (reg_kind == PG_TRAIN_REG_BCE && !fgs) return pg_fail(h, PG_EINVAL, "%s: the BCE regulariser needs fgs", who);
    if (std::isnan(base_bg) && use_background && !bgs) return pg_fail(h, PG_EINVAL, "%s: base_bg is NaN", who);
    const void* f32s[] = {rgb_map, acc_map, rgb0, acc0, target, bgs, fgs, d_rgb_map, d_acc_map, d_rgb0, d_acc0};
    for (const void* p : f32s)
        if (pg_misaligned(p, sizeof(float))) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    if (pg_misaligned(summary, sizeof(double))) return pg_fail(h, PG_EINVAL, "%s: summary is not aligned to a double", who);

    PG_HIP(h, hipSetDevice(h->device));
    State* s = nullptr;
    PG_TRY(pg_state(h, s));
    const long long nblocks = (n + THREADS - 1) / THREADS;
    PG_TRY(pg_grow(h, s->loss_part, (size_t)nblocks * NQ * sizeof(double), "training loss partial sums", (size_t)(nblocks + nblocks / 2) * NQ * sizeof(double)));
    LossArgs a{};
    a.rgb[0] = rgb_map; a.acc[0] = acc_map; a.rgb[1] = rgb0; a.acc[1] = acc0;
    a.target = target; a.bgs = use_background ? bgs : nullptr; a.fgs = fgs;
    a.n = n; a.nblocks = nblocks; a.n_pass = rgb0 ? 2 : 1;
    a.loss_kind = loss_kind; a.use_bg = use_background ? 1 : 0; a.reg_kind = reg_kind;
    a.beta = beta; a.base_bg = base_bg; a.coarse_weight = coarse_weight; a.reg_coef = reg_coef;
    a.part = s->loss_part.as<double>(); a.summary = summary;
    a.d_rgb[0] = d_rgb_map; a.d_acc[0] = d_acc_map; a.d_rgb[1] = d_rgb0; a.d_acc[1] = d_acc0;
    const int with_grads = (d_rgb_map || d_acc_map || d_rgb0 || d_acc0) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(loss_part_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "training loss kernel");
    hipLaunchKernelGGL(loss_grad_kernel, dim3(with_grads ? (unsigned)nblocks : 1u), dim3(THREADS), 0, st, a, with_grads);
    PG_LAUNCH_CHECK(h, "training loss gradient kernel");
    return PG_OK;
}

extern "C" int pg_pose_reg_loss(pg_handle* h, void* stream, int64_t n, const float* rots, const float* kps, int64_t N, const float* anchor_rots,
                                const float* anchor_kps, const int32_t* kp_idx, double tol, double coef, double ext_scale,
                                const float* prev_rots, const float* prev_kps, const float* next_rots, const float* next_kps,
                                const float* temp_val, double temp_coef, double* summary, float* d_rots, float* d_kps) {
    using namespace pgtl;
    const char* who = "pg_pose_reg_loss";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!rots || !kps || !anchor_rots || !anchor_kps || !kp_idx || !summary)
        return pg_fail(h, PG_EINVAL, "%s: rots, kps, the anchors, kp_idx and summary are required", who);
    if (n < 1 || n > 0x7fffffffll / NJ) return pg_fail(h, PG_EINVAL, "%s: n = %lld is outside [1, %lld]", who, (long long)n, 0x7fffffffll / NJ);
    if (N < 1 || N > 0x7fffffffll / NJ) return pg_fail(h, PG_EINVAL, "%s: N = %lld anchors", who, (long long)N);
    const int given = (prev_rots != nullptr) + (prev_kps != nullptr) + (next_rots != nullptr) + (next_kps != nullptr);
    if (given != 0 && given != 4) return pg_fail(h, PG_EINVAL, "%s: the temporal term takes prev / next rots and kps, all four or none", who);
    const bool temporal = given == 4;
    if (temporal && !temp_val) return pg_fail(h, PG_EINVAL, "%s: the temporal term needs temp_val", who);
    if (std::isnan(tol) || std::isnan(coef) || std::isnan(temp_coef) || !(ext_scale > 0.0))
        return pg_fail(h, PG_EINVAL, "%s: tol = %g, coef = %g, temp_coef = %g, ext_scale = %g (no NaN; ext_scale > 0)", who, tol, coef, temp_coef, ext_scale);
    const void* f32s[] = {rots, kps, anchor_rots, anchor_kps, prev_rots, prev_kps, next_rots, next_kps, temp_val, d_rots, d_kps};
    for (const void* p : f32s)
        if (pg_misaligned(p, sizeof(float))) return pg_fail(h, PG_EINVAL, "%s: an array is not aligned to its element", who);
    if (pg_misaligned(summary, sizeof(double))) return pg_fail(h, PG_EINVAL, "%s: summary is not aligned to a double", who);
    for (int64_t i = 0; i < n; ++i)
        if (kp_idx[i] < 0 || kp_idx[i] >= N) return pg_fail(h, PG_EINVAL, "%s: kp_idx[%lld] = %d is outside [0, %lld)", who, (long long)i, kp_idx[i], (long long)N);

    PG_HIP(h, hipSetDevice(h->device));
    State* s = nullptr;
    PG_TRY(pg_state(h, s));
    const long long nblocks = (n * NJ + THREADS - 1) / THREADS;
    PG_TRY(pg_grow(h, s->reg_part, (size_t)nblocks * RQ * sizeof(double), "pose regulariser partial sums", (size_t)(nblocks + nblocks / 2) * RQ * sizeof(double)));
    PG_TRY(pg_grow(h, s->d_idx, (size_t)n * sizeof(int32_t), "pose regulariser indices", (size_t)(n + n / 2) * sizeof(int32_t)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    s->host_idx.assign(kp_idx, kp_idx + n);
    PG_HIP(h, hipMemcpyAsync(s->d_idx.p, s->host_idx.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    RegArgs a{};
    a.rots = rots; a.kps = kps; a.a_rots = anchor_rots; a.a_kps = anchor_kps; a.kp_idx = s->d_idx.as<const int32_t>();
    a.p_rots = prev_rots; a.p_kps = prev_kps; a.n_rots = next_rots; a.n_kps = next_kps; a.temp_val = temp_val;
    a.n = n; a.nblocks = nblocks; a.temporal = temporal ? 1 : 0;
    a.tol = (double)(float)tol;                              // the reference compares float32 squares with the float32 of opt_pose_tol
    a.coef = coef; a.temp_coef = temp_coef; a.ext_scale = ext_scale;
    a.part = s->reg_part.as<double>(); a.summary = summary; a.d_rots = d_rots; a.d_kps = d_kps;
    hipLaunchKernelGGL(reg_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "pose regulariser kernel");
    hipLaunchKernelGGL(reg_final_kernel, dim3(1), dim3(THREADS), 0, st, a);
    PG_LAUNCH_CHECK(h, "pose regulariser sum kernel");
    return PG_OK;
}

extern "C" int pg_grad_norms(pg_handle* h, void* stream, int n_tensors, const float* const* grads, const int64_t* counts, double* out) {
    using namespace pgtl;
    const char* who = "pg_grad_norms";
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (n_tensors < 1 || n_tensors > PG_GRAD_NORMS_MAX)
        return pg_fail(h, PG_EINVAL, "%s: n_tensors = %d is outside [1, %d] (the reference divides by zero without a gradient)", who, n_tensors,
                       PG_GRAD_NORMS_MAX);
    if (!grads || !counts || !out) return pg_fail(h, PG_EINVAL, "%s: grads, counts and out are required", who);
    if (pg_misaligned(out, sizeof(double))) return pg_fail(h, PG_EINVAL, "%s: out is not aligned to a double", who);
    State* s = nullptr;
    PG_TRY(pg_state(h, s));
    s->host_tab.resize((size_t)n_tensors);
    long long nblocks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (counts[t] < 0 || (counts[t] > 0 && !grads[t])) return pg_fail(h, PG_EINVAL, "%s: tensor %d: %lld elements at %p", who, t, (long long)counts[t], (const void*)grads[t]);
        if (pg_misaligned(grads[t], sizeof(float))) return pg_fail(h, PG_EINVAL, "%s: tensor %d is not aligned to a float", who, t);
        s->host_tab[t] = NormEntry{grads[t], (long long)counts[t], nblocks};
        nblocks += ((long long)counts[t] + SEG - 1) / SEG;
        if (nblocks > 0x7fffffffll) return pg_fail(h, PG_EINVAL, "%s: more than 2^31 - 1 segments of %d elements", who, SEG);
    }
    PG_HIP(h, hipSetDevice(h->device));
    PG_TRY(pg_grow(h, s->norm_part, (size_t)(nblocks + 1) * sizeof(double), "gradient norm partial sums", (size_t)(nblocks + nblocks / 2 + 1) * sizeof(double)));
    PG_TRY(pg_grow(h, s->d_tab, (size_t)PG_GRAD_NORMS_MAX * sizeof(NormEntry), "gradient norm tensor table"));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_HIP(h, hipMemcpyAsync(s->d_tab.p, s->host_tab.data(), (size_t)n_tensors * sizeof(NormEntry), hipMemcpyHostToDevice, st));
    const NormEntry* tab = s->d_tab.as<const NormEntry>();
    if (nblocks > 0) {
        hipLaunchKernelGGL(norm_part_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, st, tab, n_tensors, s->norm_part.as<double>());
        PG_LAUNCH_CHECK(h, "gradient norm kernel");
    }
    hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(THREADS), 0, st, tab, n_tensors, s->norm_part.as<const double>(), out);
    PG_LAUNCH_CHECK(h, "gradient norm sum kernel");
    return PG_OK;
}
