// pg_optim.hip -- the optimiser step (include/posegen_optim.h): clip_grad_norm_ over the tensors of the call and
// torch.optim.Adam's update of every one of them.
//   adam_sumsq_kernel  : one workgroup per 16384-element segment of one gradient: its sum of squares in double (pg_sumsq.h, the
//                        arithmetic of pg_grad_norms) -> part[block].
//   adam_coef_kernel   : one workgroup.  Thread t takes tensors t, t + 256, ... in that order and adds each one's segments in
//                        ascending order; the 256 sums fold in a fixed tree -> out = (norm, coef).
//   adam_update_kernel : one workgroup per segment of one tensor, a pure stream: p, g, m, v in, p, m, v (and g) out, float64
//                        arithmetic from the float32 inputs, each output rounded once.  Where the four arrays share a 16-byte phase
//                        the body moves 16 bytes per access, two quads per lane in flight, behind a scalar head and in front of a
//                        scalar tail; otherwise element by element.  No LDS.
// The workgroup -> (tensor, segment) lookup is a binary search over first_block (pg_optim_plan.h).  No atomics; the split into
// partial sums depends on the sizes alone; nothing is kept between calls except grow-only scratch.  Double sqrt and division are the
// correctly rounded ones: this file is built without fast-math flags.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "pg_handle.h"
#include "pg_optim_plan.h"
#include "pg_sumsq.h"

namespace pgop {

constexpr int THREADS = pgsq::THREADS;
static_assert(SEG == pgsq::SEG, "the update and the norm cut a tensor into the same segments");

__global__ __launch_bounds__(THREADS) void adam_sumsq_kernel(const Entry* __restrict__ tab, int n, double* __restrict__ part) {
    __shared__ double lds[pgsq::SLOTS];
    const Entry& en = tab[entry_of_block(tab, n, (long long)blockIdx.x)];
    const long long off = ((long long)blockIdx.x - en.first_block) * SEG;
    const long long rest = en.count - off;
    const double sq = pgsq::segment_sumsq(en.g + off, rest < SEG ? (int)rest : SEG, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

// out[0] = |g|_2 over the call, out[1] = the coefficient clip_grad_norm_ multiplies by (1 without clipping)
__global__ __launch_bounds__(THREADS) void adam_coef_kernel(const Entry* __restrict__ tab, int n, const double* __restrict__ part, double max_norm,
                                                            int clip, double* __restrict__ out) {
    __shared__ double lds[THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int t = tid; t < n; t += THREADS) {
        const long long fb = tab[t].first_block, nb = segments_of(tab[t].count);
        double sq = 0.0;
        for (long long b = 0; b < nb; ++b) sq += part[fb + b];
        acc += sq;
    }
    lds[tid] = acc;
    __syncthreads();
    for (int d = THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) lds[tid] += lds[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        const double norm = sqrt(lds[0]);
        double coef = 1.0;
        if (clip) {
            coef = max_norm / (norm + 1e-6);
            coef = coef > 1.0 ? 1.0 : coef;                  // (torch.clamp(max=1): NaN stays NaN)
        }
        out[0] = norm;
        out[1] = coef;
    }
}

struct Out { float p, m, v, g; };

// one element: torch's _single_tensor_adam in double
__device__ __forceinline__ Out adam_element(const Entry& en, double coef, float pf, float gf, float mf, float vf) {
    const double p = (double)pf, m = (double)mf, v = (double)vf;
    const double g = coef * (double)gf;
    double gp = g;
    if (en.wd != 0.0) gp = g + en.wd * p;
    const double m1 = m + (gp - m) * en.omb1;
    const double v1 = en.beta2 * v + en.omb2 * (gp * gp);
    const double denom = sqrt(v1) / en.bc2_sqrt + en.eps;
    const double p1 = p - en.step_size * (m1 / denom);
    return Out{(float)p1, (float)m1, (float)v1, (float)g};
}

__device__ __forceinline__ void adam_quad(const Entry& en, double coef, float4& p, float4& g, float4& m, float4& v) {
    const Out a = adam_element(en, coef, p.x, g.x, m.x, v.x), b = adam_element(en, coef, p.y, g.y, m.y, v.y);
    const Out c = adam_element(en, coef, p.z, g.z, m.z, v.z), d = adam_element(en, coef, p.w, g.w, m.w, v.w);
    p = make_float4(a.p, b.p, c.p, d.p); g = make_float4(a.g, b.g, c.g, d.g);
    m = make_float4(a.m, b.m, c.m, d.m); v = make_float4(a.v, b.v, c.v, d.v);
}

__global__ __launch_bounds__(THREADS) void adam_update_kernel(const Entry* __restrict__ tab, int n, const double* __restrict__ norm_coef,
                                                              int write_grads) {
    const Entry en = tab[entry_of_block(tab, n, (long long)blockIdx.x)];
    const long long off = ((long long)blockIdx.x - en.first_block) * SEG;
    const long long rest = en.count - off;
    const int len = rest < SEG ? (int)rest : SEG;
    float* __restrict__ p = en.p + off;
    float* __restrict__ g = en.g + off;
    float* __restrict__ m = en.m + off;
    float* __restrict__ v = en.v + off;
    const double coef = norm_coef ? norm_coef[1] : 1.0;
    const int tid = threadIdx.x;
    const unsigned php = (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u, phg = (unsigned)(reinterpret_cast<uintptr_t>(g) >> 2) & 3u;
    const unsigned phm = (unsigned)(reinterpret_cast<uintptr_t>(m) >> 2) & 3u, phv = (unsigned)(reinterpret_cast<uintptr_t>(v) >> 2) & 3u;
    int lo = 0, hi = len;                                     // elements [lo, hi) go through the scalar loop below
    if (php == phg && php == phm && php == phv) {
        int head = (int)((4u - php) & 3u);                    // elements in front of the first 16-byte boundary
        if (head > len) head = len;
        const int nq = (len - head) / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p + head);
        float4* __restrict__ g4 = reinterpret_cast<float4*>(g + head);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m + head);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(v + head);
        int q = tid;
        for (; q + THREADS < nq; q += 2 * THREADS) {          // two quads per lane: eight 16-byte loads in flight
            float4 pa = p4[q], ga = g4[q], ma = m4[q], va = v4[q];
            float4 pb = p4[q + THREADS], gb = g4[q + THREADS], mb = m4[q + THREADS], vb = v4[q + THREADS];
            adam_quad(en, coef, pa, ga, ma, va);
            adam_quad(en, coef, pb, gb, mb, vb);
            p4[q] = pa; m4[q] = ma; v4[q] = va;
            p4[q + THREADS] = pb; m4[q + THREADS] = mb; v4[q + THREADS] = vb;
            if (write_grads) { g4[q] = ga; g4[q + THREADS] = gb; }
        }
        if (q < nq) {
            float4 pa = p4[q], ga = g4[q], ma = m4[q], va = v4[q];
            adam_quad(en, coef, pa, ga, ma, va);
            p4[q] = pa; m4[q] = ma; v4[q] = va;
            if (write_grads) g4[q] = ga;
        }
        // head and tail: fewer than four elements each, the first lanes take one apiece
        lo = head + 4 * nq;
        if (tid < head) {
            const Out o = adam_element(en, coef, p[tid], g[tid], m[tid], v[tid]);
            p[tid] = o.p; m[tid] = o.m; v[tid] = o.v;
            if (write_grads) g[tid] = o.g;
        }
    }
    for (int i = lo + tid; i < hi; i += THREADS) {
        const Out o = adam_element(en, coef, p[i], g[i], m[i], v[i]);
        p[i] = o.p; m[i] = o.m; v[i] = o.v;
        if (write_grads) g[i] = o.g;
    }
}

// what pg_adam_step keeps in the handle: the device table and its host copy (read by the upload while it is in flight), the
// partial sums, and the (norm, coef) pair of a clipped call without `out`.  Calls on one handle are serialised by the caller.
struct State : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_OPTIM;
    ~State() override { for (DevBuf* b : {&d_tab, &part, &norm_coef}) pg_release(*b); }
    DevBuf d_tab, part, norm_coef;
    std::vector<Entry> host_tab;
};

}  // namespace pgop

extern "C" int pg_adam_step(pg_handle* h, void* stream, int n_tensors, const pg_adam_tensor* tensors, int n_groups, const pg_adam_group* groups,
                            double max_norm, int write_grads, double* out) {
    using namespace pgop;
    const char* who = "pg_adam_step";
    char msg[320];
    if (check_tables(n_tensors, tensors, n_groups, groups, max_norm, out, msg, sizeof msg)) return pg_fail(h, PG_EINVAL, "%s: %s", who, msg);
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    State* s = nullptr;
    PG_TRY(pg_state(h, s));
    s->host_tab.resize((size_t)n_tensors);
    long long nblocks = 0;
    const int n = plan_entries(n_tensors, tensors, groups, s->host_tab.data(), &nblocks);
    const bool clip = max_norm != PG_ADAM_NO_CLIP;
    const bool want_norm = clip || out != nullptr;
    if (n == 0 && !want_norm) return PG_OK;                   // every tensor is empty
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Entry* tab = nullptr;
    if (n > 0) {
        PG_TRY(pg_grow(h, s->d_tab, (size_t)n * sizeof(Entry), "optimiser tensor table", (size_t)(n + n / 2) * sizeof(Entry)));
        PG_HIP(h, hipMemcpyAsync(s->d_tab.p, s->host_tab.data(), (size_t)n * sizeof(Entry), hipMemcpyHostToDevice, st));
        tab = s->d_tab.as<const Entry>();
    }
    const double* norm_coef = nullptr;
    if (want_norm) {
        PG_TRY(pg_grow(h, s->part, (size_t)(nblocks + 1) * sizeof(double), "optimiser partial sums", (size_t)(nblocks + nblocks / 2 + 1) * sizeof(double)));
        double* nc = out;
        if (!nc) {
            PG_TRY(pg_grow(h, s->norm_coef, 2 * sizeof(double), "optimiser clipping coefficient"));
            nc = s->norm_coef.as<double>();
        }
        if (n > 0) {
            hipLaunchKernelGGL(adam_sumsq_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, st, tab, n, s->part.as<double>());
            PG_LAUNCH_CHECK(h, "optimiser norm kernel");
        }
        hipLaunchKernelGGL(adam_coef_kernel, dim3(1), dim3(THREADS), 0, st, tab, n, s->part.as<const double>(), max_norm, clip ? 1 : 0, nc);
        PG_LAUNCH_CHECK(h, "optimiser coefficient kernel");
        if (clip) norm_coef = nc;
    }
    if (n > 0) {
        hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, st, tab, n, norm_coef, write_grads ? 1 : 0);
        PG_LAUNCH_CHECK(h, "optimiser update kernel");
    }
    return PG_OK;
}
