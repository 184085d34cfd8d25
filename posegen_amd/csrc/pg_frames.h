// pg_frames.h -- the frame front and back end of pg_frames.hip for the other translation unit that renders boxes of a frame
// (pg_scene.hip: several people in one frame): the geometry of a box, the render of a range of its rays, the composition of its
// maps into the frame.
#pragma once
#include <cstdint>

#include "pg_handle.h"
#include "pg_launch.h"

struct FrameMaps { float *rgb_map, *disp_map, *acc_map; };      // [n_box,3], [n_box], [n_box]: the whole box (each may be null: not wanted)
// what the final maps of a range are composited from, kept per ray: the depths [n,S + N] and the raw [n,S + N,4] (single_net: merged)
struct FrameLists { float *z, *raw; };

int frame_geom(pg_handle* h, int H, int W, const float* c2w, const float* intrinsics, const int* box, float near,
               float far, float cam, pgk::FrameGeom* g);
// rays [r0, r1) of the box (row-major ray list of kp_to_valid_rays).  r0 must be a multiple of the nanmean
// group size (`chunk`) unless it is 0, so that the groups are those of the whole frame.  ext == nullptr:
// the maps of the whole box are carved from the frame workspace and the range is written at its offset
// (returned in *maps); otherwise the range's maps go to ext (rgb [r1-r0,3], disp, acc [r1-r0]).  lists: the range's
// sample lists as well ([r1-r0, ...]).
int frame_render_range(pg_handle* h, void* stream, const pgk::FrameGeom& g, int64_t r0, int64_t r1, const float* skts,
                       const float* cyl, int n_samples, int n_importance, int flags, FrameMaps* maps, const FrameMaps* ext = nullptr,
                       const FrameLists* lists = nullptr);
int frame_compose(pg_handle* h, void* stream, const pgk::FrameGeom& g, const FrameMaps& maps, const float* bg, float base_bg,
                  float* rgb, float* disp, float* acc, uint8_t* rgb8);
