// pg_frame_dir.h -- the direction of the ray through pixel (row r, column c) of a frame: the ONE device function behind
// frame_rays_kernel (pg_kernels.hip), which writes it into the ray_batch rows a frame is rendered from, and
// scene_composite_kernel (pg_scene.hip), which needs the norm of that same vector again when it merges several people's
// sample lists of a pixel.  get_rays (core/utils/ray_utils.py:6-28): plain fp32 ops in the reference's order, no FMA.
#pragma once
#include <hip/hip_runtime.h>

#include "pg_launch.h"

namespace pgk {

__device__ __forceinline__ void frame_ray_dir(const FrameGeom& g, int r, int c, float d[3]) {
    const float dx = __fdiv_rn(__fsub_rn((float)c, g.cx), g.fx);
    const float dy = -__fdiv_rn(__fsub_rn((float)r, g.cy), g.fy);
    const float dz = -1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        d[k] = __fadd_rn(__fadd_rn(__fmul_rn(dx, g.R[3 * k]), __fmul_rn(dy, g.R[3 * k + 1])), __fmul_rn(dz, g.R[3 * k + 2]));
}

}  // namespace pgk
