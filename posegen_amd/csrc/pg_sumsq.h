// pg_sumsq.h -- the sum of squares of one segment of a float32 tensor in double, in a fixed order: what norm_part_kernel
// (pg_trainloss.hip, pg_grad_norms) and the clipping norm of pg_adam_step (pg_optim.hip) share.  Element i of a segment always lands
// in slot i mod 1024, whatever the pointer's alignment: the aligned 16-byte loads start `m` elements in front of the segment
// (m = 0..3), head and tail quads are read element by element, and thread t's four accumulators are slots (4 t + c - m) mod 1024.
// The 1024 slots fold in a fixed tree.  Device code; included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgsq {

constexpr int THREADS = 256;
constexpr int SEG = 16384;        // elements of one workgroup
constexpr int SLOTS = 4 * THREADS;

// the sum of base[0 .. len)^2, len <= SEG, by a workgroup of THREADS threads; lds: SLOTS doubles.  Valid in every thread on return.
__device__ __forceinline__ double segment_sumsq(const float* __restrict__ base, int len, double* lds) {
    const int tid = threadIdx.x;
    const int m = (int)((reinterpret_cast<uintptr_t>(base) >> 2) & 3);   // elements between the 16-byte boundary below `base` and `base`
    const float4* quads = reinterpret_cast<const float4*>(base - m);
    const int end = m + len;                                             // positions [m, end) are the segment's elements
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = tid; 4 * q < end; q += THREADS) {
        const int p0 = 4 * q;
        if (p0 >= m && p0 + 4 <= end) {
            const float4 f = quads[q];
            acc[0] += (double)f.x * (double)f.x; acc[1] += (double)f.y * (double)f.y;
            acc[2] += (double)f.z * (double)f.z; acc[3] += (double)f.w * (double)f.w;
        } else {                                                         // the head and the tail quad: only the elements inside
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int p = p0 + c;
                if (p >= m && p < end) { const double f = (double)base[p - m]; acc[c] += f * f; }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[(4 * tid + c - m + SLOTS) % SLOTS] = acc[c];     // element i of the segment is in slot i mod 1024
    __syncthreads();
    for (int d = SLOTS / 2; d >= 1; d >>= 1) {
        for (int k = tid; k < d; k += THREADS) lds[k] += lds[k + d];
        __syncthreads();
    }
    return lds[0];
}

}  // namespace pgsq
