// pg_optim_plan.h -- what pg_adam_step (pg_optim.hip) decides on the host before it launches: the check of its two
// tables, the device table with one entry per non-empty tensor (the hyperparameters of its group and the bias corrections of its
// step, formed here in double), the count of segments against the grid limit, the prefix `first_block`, and the lookup workgroup ->
// (tensor, segment) that the kernels run as well.  Free of HIP calls, like pg_metrics_plan.h, so that it compiles into a plain C++
// program (tools/sanitize/optim_plan_asan.cpp, built with the address and undefined-behaviour sanitisers).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/posegen_optim.h"

#if defined(__HIPCC__)
#define PG_OPTIM_HD __host__ __device__
#else
#define PG_OPTIM_HD
#endif

namespace pgop {

constexpr int SEG = PG_ADAM_SEGMENT;
constexpr long long MAX_BLOCKS = 0x7fffffffll;       // a grid's x extent

// One non-empty tensor as the kernels see it.
struct Entry {
    float* p;
    float* g;
    float* m;
    float* v;
    long long count;
    long long first_block;       // the tensor's segments are workgroups first_block .. first_block + segments_of(count) - 1
    double wd, omb1, beta2, omb2, eps;
    double step_size;            // lr / (1 - beta1^t)
    double bc2_sqrt;             // sqrt(1 - beta2^t)
};

PG_OPTIM_HD inline long long segments_of(long long count) { return (count + SEG - 1) / SEG; }

// The entry that owns workgroup `block`, 0 <= block < the total of the n entries' segments (n >= 1, every entry non-empty): the
// last one whose first_block is <= block.
PG_OPTIM_HD inline int entry_of_block(const Entry* tab, int n, long long block) {
    int lo = 0, hi = n - 1;                              // the answer is in [lo, hi]
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].first_block <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

inline bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

// The refusals of pg_adam_step: 0, or -1 with the reason in msg.
inline int check_tables(int n_tensors, const pg_adam_tensor* tensors, int n_groups, const pg_adam_group* groups, double max_norm,
                        const double* out, char* msg, size_t cap) {
    if (n_tensors < 1 || n_tensors > PG_ADAM_MAX_TENSORS) { std::snprintf(msg, cap, "n_tensors = %d is outside [1, %d]", n_tensors, PG_ADAM_MAX_TENSORS); return -1; }
    if (n_groups < 1 || n_groups > PG_ADAM_MAX_GROUPS) { std::snprintf(msg, cap, "n_groups = %d is outside [1, %d]", n_groups, PG_ADAM_MAX_GROUPS); return -1; }
    if (!tensors || !groups) { std::snprintf(msg, cap, "tensors and groups are required"); return -1; }
    if (std::isnan(max_norm) || (max_norm < 0.0 && max_norm != PG_ADAM_NO_CLIP)) { std::snprintf(msg, cap, "max_norm = %g (PG_ADAM_NO_CLIP or >= 0)", max_norm); return -1; }
    if (misaligned(out, sizeof(double))) { std::snprintf(msg, cap, "out is not aligned to a double"); return -1; }
    for (int k = 0; k < n_groups; ++k) {
        const pg_adam_group& q = groups[k];
        if (!(q.lr >= 0.0) || !(q.eps >= 0.0) || !(q.beta1 >= 0.0 && q.beta1 < 1.0) || !(q.beta2 >= 0.0 && q.beta2 < 1.0) || !(q.weight_decay >= 0.0)) {
            std::snprintf(msg, cap, "group %d: lr = %g, betas = (%g, %g), eps = %g, weight_decay = %g (lr, eps, weight_decay >= 0; 0 <= beta < 1)", k,
                          q.lr, q.beta1, q.beta2, q.eps, q.weight_decay);
            return -1;
        }
    }
    long long nblocks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const pg_adam_tensor& e = tensors[t];
        if (e.group < 0 || e.group >= n_groups) { std::snprintf(msg, cap, "tensor %d: group %d is outside [0, %d)", t, e.group, n_groups); return -1; }
        if (e.step < 1) { std::snprintf(msg, cap, "tensor %d: step = %d (the step being taken, >= 1)", t, e.step); return -1; }
        if (e.count < 0) { std::snprintf(msg, cap, "tensor %d: %lld elements", t, (long long)e.count); return -1; }
        const void* ptrs[4] = {e.param, e.grad, e.exp_avg, e.exp_avg_sq};
        for (const void* p : ptrs) {
            if (e.count > 0 && !p) { std::snprintf(msg, cap, "tensor %d: a NULL pointer with %lld elements", t, (long long)e.count); return -1; }
            if (misaligned(p, sizeof(float))) { std::snprintf(msg, cap, "tensor %d: a pointer is not aligned to a float", t); return -1; }
        }
        if (e.count > MAX_BLOCKS * SEG) { std::snprintf(msg, cap, "more than 2^31 - 1 segments of %d elements", SEG); return -1; }
        nblocks += segments_of(e.count);
        if (nblocks > MAX_BLOCKS) { std::snprintf(msg, cap, "more than 2^31 - 1 segments of %d elements", SEG); return -1; }
    }
    return 0;
}

// The device table of checked tables: `tab` has room for n_tensors entries; returns how many it filled (the non-empty tensors, in
// the caller's order) and the total of their segments in *nblocks.
inline int plan_entries(int n_tensors, const pg_adam_tensor* tensors, const pg_adam_group* groups, Entry* tab, long long* nblocks) {
    int n = 0;
    long long nb = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const pg_adam_tensor& e = tensors[t];
        if (e.count == 0) continue;
        const pg_adam_group& q = groups[e.group];
        Entry& en = tab[n++];
        en.p = e.param; en.g = e.grad; en.m = e.exp_avg; en.v = e.exp_avg_sq;
        en.count = e.count;
        en.first_block = nb;
        en.wd = q.weight_decay; en.omb1 = 1.0 - q.beta1; en.beta2 = q.beta2; en.omb2 = 1.0 - q.beta2; en.eps = q.eps;
        en.step_size = q.lr / (1.0 - std::pow(q.beta1, (double)e.step));
        en.bc2_sqrt = std::sqrt(1.0 - std::pow(q.beta2, (double)e.step));
        nb += segments_of(e.count);
    }
    *nblocks = nb;
    return n;
}

}  // namespace pgop
