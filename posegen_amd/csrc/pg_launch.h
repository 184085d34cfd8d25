// pg_launch.h -- the ONE declaration of every launcher and query the translation units call in each other, and of the host-side
// structs that cross those calls.  Every file that calls one and every file that defines one includes it: with C linkage nothing
// else checks a definition against its callers (one that drifts from its declaration is a conflicting-types error where it is defined).
#pragma once
#include <cstdint>

#include "../../include/posegen_hip.h"

namespace pgd { struct EvalArgs; struct RecArgs; }      // pg_device.h
namespace pgkin { struct KinTree; }                     // pg_kin.h

namespace pgk {

// frame front / back end (frame_rays_kernel, frame_compose_kernel: passed by value as a kernel argument)
struct FrameGeom {
    int H, W, tlx, tly, bw, bh;        // box = pixels [tly, tly+bh) x [tlx, tlx+bw)
    float fx, fy, cx, cy;
    float R[9], t[3];                   // c2w[:3,:3] row-major, c2w[:3,3]
    float near, far, cam;
};

// raw2outputs' density: sigma = act(raw.w / scale + noise), colours within [-rgb_eps, 1 + rgb_eps]
struct Density { float scale, rgb_eps; int act; float shift; };
inline Density density_of(const pg_config& c) { return {c.density_scale, c.rgb_eps, c.density_act, c.softplus_shift}; }

struct Maps { float *rgb, *disp, *acc, *alpha; };      // [n,3], [n], [n], [n,S]; each may be null
inline Maps final_maps(const pg_outputs& o) { return {o.rgb_map, o.disp_map, o.acc_map, o.alpha}; }
inline Maps coarse_maps(const pg_outputs& o) { return {o.rgb0, o.disp0, o.acc0, o.alpha0}; }

// One compositing launch (composite_kernel, pg_kernels.hip): a caller fills the first block and whatever else it means.
struct Composite {
    const float *rays, *z, *raw;        // [n,11], depths [n,S], [n,S,4] (pg_launch_composite_merged: the coarse points' [n,S - n_imp,4])
    long long n;
    int S;
    Density den;
    Maps out;
    const float* noise = nullptr;       // density noise [n,S]
    float* weights = nullptr;           // [n,S]
    // importance sampling: n_imp new depths per ray from the weights' pdf (deterministic, or at the draws u_rand [n,n_imp]), merged
    // with z into z_fine [n,S + n_imp]; order [n,S + n_imp] (may be null) receives the sort permutation
    int n_imp = 0;
    float* z_fine = nullptr;
    const float* u_rand = nullptr;
    int* order = nullptr;
    // pg_launch_composite_iso (single_net, coarse pass): the is_only pdf; z_new [n,ld_new] (may be null) receives the new depths in
    // sample order (columns n_imp.. repeat the last one)
    float* z_new = nullptr;
    int ld_new = 0;
    // pg_launch_composite_merged (single_net, fine pass over z = z_fine): sample s reads raw[order] or raw_new[order - (S - n_imp)]
    // (order: the map pg_launch_composite_iso wrote; raw_new [n,ld_new,4]); raw_out [n,S,4] (may be null) receives the merged raw
    const float* raw_new = nullptr;
    float* raw_out = nullptr;
};

// One gather launch of a training batch (batch_gather_kernel, pg_batch.hip: passed by value as a kernel argument)
struct BatchGather {
    const uint8_t *imgs, *masks, *bkgds;    // [F,P,3], [F,P], [n_bkgd,P,3] (may be null)
    const float *c2ws, *focals, *centers;   // [n_cam,3,4], [n_cam,2] = (fx, fy), [n_cam,2] = (cx, cy) (may be null)
    long long P;
    int H, W, mask_img;
    const int* rows;                        // [3,n_img]: image row, camera row, background row of every batch image
    long long n_img;
    int k;
    const int* pix;                         // [n_img k] flat pixel ids
    float *target, *fgs, *bgs, *rays_o, *rays_d, *ray_batch;       // [n,3], [n], [n,3] (may be null), [n,3], [n,3], [n,11]
};

}  // namespace pgk

extern "C" {
// ---- the fused eval kernels and the per-ray record kernel in front of them (pg_eval*.hip, pg_rayrec.hip) ----
int pg_launch_eval16(const pgd::EvalArgs* a, int fp16, int framecode, int grid, void* stream);
int pg_launch_eval16r(const pgd::EvalArgs* a, int fp16, int framecode, int onchip, int grid, void* stream);
int pg_launch_eval32(const pgd::EvalArgs* a, int precision, int framecode, int grid, void* stream);
int pg_launch_evalc2(const pgd::EvalArgs* a, int framecode, int grid, void* stream);
int pg_launch_ray_records(const pgd::RecArgs* a, int fp16, int framecode, int n_cu, void* stream);
int pg_eval16_points_per_pass(void);
int pg_eval16_wgs_per_cu(void);
int pg_eval32_points_per_pass(void);
int pg_evalc2_points_per_pass(void);
// ---- pg_kernels.hip: sampling, compositing, poses, frames, calibration ----
int pg_launch_sample_coarse(const float* rays, const float* cyls, long long cyl_stride, long long n, int chunk, int S, int lindisp, float* near_far,
                            float* z, const float* t_rand, double* scratch, void* stream);
long long pg_sample_coarse_scratch(long long n, int chunk);
int pg_launch_gather_noise(const float* src, long long n, int stride, int S, const int* order, float* dst, void* stream);
int pg_launch_composite(const pgk::Composite* c, void* stream);
int pg_launch_composite_iso(const pgk::Composite* c, void* stream);
int pg_launch_composite_merged(const pgk::Composite* c, void* stream);
int pg_composite_max_samples(void);
int pg_composite_max_importance(void);
int pg_launch_mfma_rate(int f16, int lds_fed, int blocks, int iters, float* sink, void* stream);
int pg_launch_frame_rays(const pgk::FrameGeom* g, long long i0, long long n, float* rays, float* cams, void* stream);
int pg_launch_frame_compose(const pgk::FrameGeom* g, const float* rgb_map, const float* disp_map, const float* acc_map,
                            const float* bg, float base_bg, float* rgb, float* disp, float* acc, uint8_t* rgb8, void* stream);
int pg_launch_pose_kinematics(const double* offs72, const pgkin::KinTree* tree, const double* bones, long long n,
                              float* kps, float* skts, double* l2ws, void* stream);
int pg_launch_pose_boxes(const float* kps, long long n, const double* w2c, long long w2c_stride, const double* ring,
                         float ext_r, float ext_top, float ext_bot, double fx, double fy, int H, int W, int offx, int offy,
                         float* cyls, int* boxes, void* stream);
// ---- pg_mesh.hip: the density grid as input of the fused eval kernels ----
int pg_launch_grid_rays(const float* root3, const float* t, int R, long long row0, long long rows, float* rays, float* z, void* stream);
int pg_launch_grid_points(const float* root3, const float* t, int R, long long p0, long long n, float* pts, void* stream);
int pg_launch_gather_sigma(const float* raw, long long n, float* sigma, void* stream);
// ---- pg_batch.hip: training batches from an image bank on the device ----
int pg_batch_tile_pixels(void);
int pg_batch_max_pixels(void);
// tile_cnt [F ceil(P / tile)]: the tiles' counts, left as each image's exclusive prefix; counts [F]
int pg_launch_pixel_count(const uint8_t* masks, long long F, long long P, int* tile_cnt, long long* counts, void* stream);
int pg_launch_pixel_emit(const uint8_t* masks, long long F, long long P, const int* tile_off, const long long* start, int* ids, void* stream);
int pg_launch_sample_pixels(const int* ids, const long long* start, const int* img_rows, long long n_img, int k, const double* draws, int* pix,
                            void* stream);
int pg_launch_batch_gather(const pgk::BatchGather* g, void* stream);
// ---- pg_repack.hip: packed images re-formed on the device (pg_load_weights_device) ----
void pg_launch_collect(const float* const* tensors, const long long* off25, float* dst, void* stream);
void pg_launch_fold(float* src, long long off_view_w, int vcols, long long off_view_b, long long off_feat_w, long long off_feat_b,
                    long long off_fw, long long off_fb, void* stream);
void pg_launch_gather16(const int32_t* map, const float* src, uint16_t* out, long long n, int is_bf, void* stream);
void pg_launch_gather32(const int32_t* map, const float* src, float* out, long long n, void* stream);
void pg_launch_codes(const float* codes, int n_codes, float* out, void* stream);
void pg_launch_ycode(const float* view_w, int vcols, const float* codes, int n_codes, float* yc, void* stream);
void pg_launch_widen_views(const float* src, int framecode_ch, float* dst, void* stream);
}
