// pg_mesh.hip -- mesh extraction around the fused eval kernels:
//   grid_rays_kernel / grid_points_kernel : the (res+1)^3 density grid as a ray batch (a grid row is a ray: o = root + (t[ix], t[iy], 0),
//                                           d = (0, 0, 1), z = t) or, where the ray form does not apply, as explicit points
//   gather_sigma_kernel                   : raw[...][3] of a slab -> the contiguous grid sigma[ix][iy][iz]
//   mc_* kernels                          : marching cubes on a device float grid [Nx,Ny,Nz]: flags and counts, two exclusive scans
//                                           (hipcub), then vertices and triangles.  Every output slot comes from a scan: no atomics, two
//                                           runs give the same bytes.
// and the two entry points that need nothing else of the renderer: pg_mesh_count, pg_mesh_emit.
// All plain fp32 vector code; byte movers with one coalesced pass over their inputs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>

#include "pg_handle.h"
#include "pg_launch.h"
#include "pg_mesh_table.inc"        // generated from posegen_amd/mesh.py by the Makefile: PG_MC_MAX_TRI, PG_MC_TRI_TABLE, PG_MC_N_TRI

namespace pgm {

constexpr int THREADS = 256;
constexpr long long MAX_POINTS = 400000000ll;      // 3 N vertices and 5 N triangles stay below 2^31: the scans are 32-bit

__device__ const signed char TRI_TABLE[256][3 * PG_MC_MAX_TRI] = {PG_MC_TRI_TABLE};
__device__ const unsigned char N_TRI[256] = {PG_MC_N_TRI};
static_assert(PG_MC_MAX_TRI <= 5, "MAX_POINTS assumes at most five triangles per cell");

// ---- the density grid as input of the fused eval kernels ---------------------------------------------------------------------
// rows [row0, row0 + rows) of the R x R rows (row = ix R + iy): rays [rows,11] = (o, d, near 0, far 1, viewdir) and z [rows,R] = t.
// p = o + d z in the eval kernels is then root + (t[ix], t[iy], t[iz]) bit for bit: d = (0, 0, 1) adds +0 to x and y, 1 z is exact.
__global__ __launch_bounds__(THREADS) void grid_rays_kernel(float rx, float ry, float rz, const float* __restrict__ t, int R,
                                                            long long row0, long long rows, float* __restrict__ rays,
                                                            float* __restrict__ z) {
    const long long tot = rows * R;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < tot; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / R;
        const int k = (int)(i - r * R);
        z[i] = t[k];
        if (k == 0) {
            const long long row = row0 + r;
            const int ix = (int)(row / R), iy = (int)(row - (long long)ix * R);
            float* q = rays + r * 11;
            q[0] = __fadd_rn(rx, t[ix]); q[1] = __fadd_rn(ry, t[iy]); q[2] = rz;
            q[3] = 0.0f; q[4] = 0.0f; q[5] = 1.0f;
            q[6] = 0.0f; q[7] = 1.0f;
            q[8] = 0.0f; q[9] = 0.0f; q[10] = 1.0f;
        }
    }
}

// points [p0, p0 + n) of the grid in its own order (iz fastest) -> pts [n,3]: the same three fp32 adds
__global__ __launch_bounds__(THREADS) void grid_points_kernel(float rx, float ry, float rz, const float* __restrict__ t, int R,
                                                              long long p0, long long n, float* __restrict__ pts) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long p = p0 + i;
        const long long row = p / R;
        const int iz = (int)(p - row * R);
        const int ix = (int)(row / R), iy = (int)(row - (long long)ix * R);
        pts[i * 3] = __fadd_rn(rx, t[ix]); pts[i * 3 + 1] = __fadd_rn(ry, t[iy]); pts[i * 3 + 2] = __fadd_rn(rz, t[iz]);
    }
}

__global__ __launch_bounds__(THREADS) void gather_sigma_kernel(const float* __restrict__ raw, long long n, float* __restrict__ sigma) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        sigma[i] = raw[i * 4 + 3];
}

// ---- marching cubes ------------------------------------------------------------------------------------------------------------
struct Dims {
    int nx, ny, nz;
    __host__ __device__ long long count() const { return (long long)nx * ny * nz; }
};

// np.maximum(v, clamp): a NaN stays a NaN (and is outside)
__device__ __forceinline__ float field(const float* __restrict__ g, long long i, float clamp) {
    const float v = g[i];
    return v < clamp ? clamp : v;
}

// per point i: which of its three edges (towards +axis 0, 1, 2) carry a vertex, the case of the cell whose lowest point it is, and the
// two counts the scans run over.  Element N of the count arrays is zero: its exclusive-scan entry is the total.
__global__ __launch_bounds__(THREADS) void mc_count_kernel(const float* __restrict__ g, Dims d, float thr, float clamp,
                                                           unsigned char* __restrict__ flags, unsigned char* __restrict__ cases,
                                                           int* __restrict__ ecnt, int* __restrict__ tcnt) {
    const long long N = d.count();
    const long long sy = d.nz, sx = (long long)d.ny * d.nz;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i <= N; i += (long long)gridDim.x * blockDim.x) {
        if (i == N) { ecnt[N] = 0; tcnt[N] = 0; continue; }
        const int ix = (int)(i / sx);
        const long long rem = i - ix * sx;
        const int iy = (int)(rem / sy), iz = (int)(rem - iy * sy);
        const bool hx = ix + 1 < d.nx, hy = iy + 1 < d.ny, hz = iz + 1 < d.nz;
        const bool in0 = field(g, i, clamp) > thr;
        unsigned fl = 0;
        if (hx && (field(g, i + sx, clamp) > thr) != in0) fl |= 1u;
        if (hy && (field(g, i + sy, clamp) > thr) != in0) fl |= 2u;
        if (hz && (field(g, i + 1, clamp) > thr) != in0) fl |= 4u;
        unsigned cs = 0;
        if (hx && hy && hz) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {       // corner c = offsets (c & 1, c >> 1 & 1, c >> 2 & 1) on axes (0, 1, 2)
                const long long j = i + (c & 1) * sx + (c >> 1 & 1) * sy + (c >> 2 & 1);
                cs |= (field(g, j, clamp) > thr ? 1u : 0u) << c;
            }
        }
        flags[i] = (unsigned char)fl;
        cases[i] = (unsigned char)cs;
        ecnt[i] = __popc(fl);
        tcnt[i] = N_TRI[cs];
    }
}

// vertices: for the edge from point i to i + 1 along axis a, tt = (thr - fa) / (fb - fa), coordinate i + tt on that axis.  The slots
// come from the stored flags and their scan alone, so a grid that changed since the count cannot move a store out of bounds.
__global__ __launch_bounds__(THREADS) void mc_vertices_kernel(const float* __restrict__ g, Dims d, float thr, float clamp,
                                                              const unsigned char* __restrict__ flags, const int* __restrict__ eoff,
                                                              float* __restrict__ verts) {
    const long long N = d.count();
    const long long sy = d.nz, sx = (long long)d.ny * d.nz;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const unsigned fl = flags[i];
        if (!fl) continue;
        const int ix = (int)(i / sx);
        const long long rem = i - ix * sx;
        const int iy = (int)(rem / sy), iz = (int)(rem - iy * sy);
        const float fa = field(g, i, clamp);
        long long slot = eoff[i];
        const float base[3] = {(float)ix, (float)iy, (float)iz};
        const long long step[3] = {sx, sy, 1};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(fl >> a & 1u)) continue;
            const float fb = field(g, i + step[a], clamp);
            const float tt = __fdiv_rn(__fsub_rn(thr, fa), __fsub_rn(fb, fa));
            float* v = verts + slot * 3;
            v[0] = a == 0 ? __fadd_rn(base[0], tt) : base[0];
            v[1] = a == 1 ? __fadd_rn(base[1], tt) : base[1];
            v[2] = a == 2 ? __fadd_rn(base[2], tt) : base[2];
            ++slot;
        }
    }
}

// triangles of the cell at point i, in table order.  Edge e = 4 a + k runs along axis a from the point offset by (k & 1) on the lower
// and (k >> 1) on the higher of the other two axes; its vertex is that point's slot plus the point's flagged edges of lower axes.
__global__ __launch_bounds__(THREADS) void mc_triangles_kernel(Dims d, const unsigned char* __restrict__ flags,
                                                               const unsigned char* __restrict__ cases, const int* __restrict__ eoff,
                                                               const int* __restrict__ toff, int* __restrict__ tris) {
    const long long N = d.count();
    const long long sy = d.nz, sx = (long long)d.ny * d.nz;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const unsigned cs = cases[i];
        const int n = N_TRI[cs];
        if (!n) continue;
        int* out = tris + (long long)toff[i] * 3;
        for (int k = 0; k < 3 * n; ++k) {
            const int e = TRI_TABLE[cs][k];
            const int a = e >> 2, lo = e & 1, hi = e >> 1 & 1;
            const long long su = a == 0 ? sy : sx, sv = a == 2 ? sy : 1;     // strides of the lower / higher of the other two axes
            const long long p = i + lo * su + hi * sv;
            out[k] = eoff[p] + __popc(flags[p] & ((1u << a) - 1u));
        }
    }
}

unsigned blocks_for(long long n) {
    const long long b = (n + THREADS - 1) / THREADS;
    return (unsigned)(b < 1 ? 1 : b < 16384 ? b : 16384);
}

// what pg_mesh_count leaves in the handle for pg_mesh_emit
struct MeshState : ModuleState {
    static constexpr ModuleSlot SLOT = MOD_MESH;
    ~MeshState() override { pg_release(arrays); pg_release(tmp); }
    DevBuf arrays;                      // the six arrays below (carve)
    unsigned char* flags = nullptr;     // [N]
    unsigned char* cases = nullptr;     // [N]
    int* ecnt = nullptr;                // [N + 1] each: counts and their exclusive scans
    int* tcnt = nullptr;
    int* eoff = nullptr;
    int* toff = nullptr;
    DevBuf tmp;                         // hipcub's scratch
    bool valid = false;                 // the scans are those of (dims, thr, clamp)
    Dims dims{0, 0, 0};
    float thr = 0.0f, clamp = 0.0f;
    long long nv = 0, nt = 0;
};

void carve(MeshState* s, Carver& c, size_t N) {
    s->flags = c.take<unsigned char>(N);
    s->cases = c.take<unsigned char>(N);
    for (int** p : {&s->ecnt, &s->tcnt, &s->eoff, &s->toff}) *p = c.take<int>(N + 1);
}

bool same_float(float a, float b) { return a == b || (a != a && b != b); }

}  // namespace pgm

extern "C" {

int pg_launch_grid_rays(const float* root3, const float* t, int R, long long row0, long long rows, float* rays, float* z, void* stream) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(pgm::grid_rays_kernel, dim3(pgm::blocks_for(rows * R)), dim3(pgm::THREADS), 0, static_cast<hipStream_t>(stream),
                       root3[0], root3[1], root3[2], t, R, row0, rows, rays, z);
    return (int)hipGetLastError();
}

int pg_launch_grid_points(const float* root3, const float* t, int R, long long p0, long long n, float* pts, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pgm::grid_points_kernel, dim3(pgm::blocks_for(n)), dim3(pgm::THREADS), 0, static_cast<hipStream_t>(stream),
                       root3[0], root3[1], root3[2], t, R, p0, n, pts);
    return (int)hipGetLastError();
}

int pg_launch_gather_sigma(const float* raw, long long n, float* sigma, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pgm::gather_sigma_kernel, dim3(pgm::blocks_for(n)), dim3(pgm::THREADS), 0, static_cast<hipStream_t>(stream), raw, n, sigma);
    return (int)hipGetLastError();
}

int pg_mesh_count(pg_handle* h, void* stream, const float* grid, int nx, int ny, int nz, float threshold, float clamp,
                  int64_t* n_vertices, int64_t* n_triangles) {
    using namespace pgm;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!grid || !n_vertices || !n_triangles) return pg_fail(h, PG_EINVAL, "pg_mesh_count: null argument");
    if (nx < 2 || ny < 2 || nz < 2) return pg_fail(h, PG_EINVAL, "pg_mesh_count: every grid dimension must be >= 2, got %d x %d x %d", nx, ny, nz);
    const Dims d{nx, ny, nz};
    const long long N = d.count();
    if (N > MAX_POINTS) return pg_fail(h, PG_EINVAL, "pg_mesh_count: at most %lld grid points per call, got %lld", MAX_POINTS, N);
    if (threshold != threshold || clamp != clamp) return pg_fail(h, PG_EINVAL, "pg_mesh_count: threshold / clamp is NaN");
    PG_HIP(h, hipSetDevice(h->device));
    MeshState* s = nullptr;
    PG_TRY(pg_state(h, s));
    s->valid = false;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Carver sizes;
    carve(s, sizes, (size_t)N);
    PG_TRY(pg_grow(h, s->arrays, sizes.off, "marching cubes scratch"));
    Carver c{s->arrays.p};
    carve(s, c, (size_t)N);
    size_t need = 0;
    PG_HIP(h, hipcub::DeviceScan::ExclusiveSum(nullptr, need, s->ecnt, s->eoff, (int)(N + 1), st));
    PG_TRY(pg_grow(h, s->tmp, need, "scan scratch"));
    hipLaunchKernelGGL(mc_count_kernel, dim3(blocks_for(N + 1)), dim3(THREADS), 0, st, grid, d, threshold, clamp, s->flags, s->cases, s->ecnt, s->tcnt);
    PG_HIP(h, hipGetLastError());
    size_t tb = s->tmp.bytes;
    PG_HIP(h, hipcub::DeviceScan::ExclusiveSum(s->tmp.p, tb, s->ecnt, s->eoff, (int)(N + 1), st));
    tb = s->tmp.bytes;
    PG_HIP(h, hipcub::DeviceScan::ExclusiveSum(s->tmp.p, tb, s->tcnt, s->toff, (int)(N + 1), st));
    int tot[2] = {0, 0};
    PG_HIP(h, hipMemcpyAsync(&tot[0], s->eoff + N, sizeof(int), hipMemcpyDeviceToHost, st));
    PG_HIP(h, hipMemcpyAsync(&tot[1], s->toff + N, sizeof(int), hipMemcpyDeviceToHost, st));
    PG_HIP(h, hipStreamSynchronize(st));
    s->dims = d; s->thr = threshold; s->clamp = clamp; s->nv = tot[0]; s->nt = tot[1]; s->valid = true;
    *n_vertices = s->nv;
    *n_triangles = s->nt;
    return PG_OK;
}

int pg_mesh_emit(pg_handle* h, void* stream, const float* grid, int nx, int ny, int nz, float threshold, float clamp, float* vertices,
                 int32_t* triangles, int64_t nv, int64_t nt) {
    using namespace pgm;
    if (!h) return pg_fail(nullptr, PG_EINVAL, "null handle");
    if (!grid) return pg_fail(h, PG_EINVAL, "pg_mesh_emit: null grid");
    const MeshState* s = h->mods.peek<MeshState>();
    if (!s || !s->valid || s->dims.nx != nx || s->dims.ny != ny || s->dims.nz != nz || !same_float(s->thr, threshold) || !same_float(s->clamp, clamp))
        return pg_fail(h, PG_ESTATE, "pg_mesh_emit: no pg_mesh_count of this grid shape, threshold and clamp precedes the call");
    if (nv != s->nv || nt != s->nt)
        return pg_fail(h, PG_ESTATE, "pg_mesh_emit: %lld vertices / %lld triangles given, the last pg_mesh_count found %lld / %lld",
                       (long long)nv, (long long)nt, s->nv, s->nt);
    if ((nv > 0 && !vertices) || (nt > 0 && !triangles)) return pg_fail(h, PG_EINVAL, "pg_mesh_emit: null output");
    PG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long N = s->dims.count();
    if (nv > 0) {
        hipLaunchKernelGGL(mc_vertices_kernel, dim3(blocks_for(N)), dim3(THREADS), 0, st, grid, s->dims, threshold, clamp, s->flags, s->eoff, vertices);
        PG_HIP(h, hipGetLastError());
    }
    if (nt > 0) {
        hipLaunchKernelGGL(mc_triangles_kernel, dim3(blocks_for(N)), dim3(THREADS), 0, st, s->dims, s->flags, s->cases, s->eoff, s->toff, triangles);
        PG_HIP(h, hipGetLastError());
    }
    return PG_OK;
}

}  // extern "C"
