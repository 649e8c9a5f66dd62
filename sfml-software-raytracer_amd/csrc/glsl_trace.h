// glsl_trace.h -- launch record shared by the GLSL-mode host mirror
// (sfrt_glsl.cpp) and its gfx950 kernel (glsl_trace.hip).  SURVEY 8f row f1.
//
// rayShader.frag (/root/reference/Raytracing/rayShader.frag) recomputes per
// fragment several terms that depend only on the uniforms; the host evaluates
// them once per draw with the same expressions:
//  * the camera basis of main() (:165-169, sin/cos) and fov.x / size.x * 2;
//  * per wall sphere the exact squared-length bound of the containment test
//    `step(length(rpos), r)` (:74), so the wall pass needs no sqrt to decide;
//  * per (light, shadow ball) pair distance(light, ball), atan(r, distance)
//    and the unit light->ball direction (:140-142).
#pragma once

#include <stdint.h>

namespace sfrt {

constexpr int kGlslMax = 100;          // uniform vec4 spheres[100] (rayShader.frag:6-8)
constexpr int kGlslMipLevels = 16;
constexpr int kGlslMarchCap = 1 << 20; // the shader has no cap; the status reports hitting it

struct GlslWall {                      // spheres[0 .. sphereCount)
  float x, y, z, r;
  float rr;                            // r*r (:77)
  float s_in;                          // step(sqrt(s), r) == 1  <=>  s <= s_in
  float pad0, pad1;
};

struct GlslBall {                      // spheres[sphereCount .. allSpheresCount)
  float x, y, z, r;
  float r_skip;                        // RU(r * (1+6e-6)) when r >= 0 (the march's dominance test), else NaN
  float pad0, pad1, pad2;
};

struct GlslPair {                      // light i, shadow ball j (:140-142)
  float dist;                          // distance(spheres[i], spheres[j])
  float sanglet;                       // atan(spheres[j].w, dist)
  float ux, uy, uz;                    // (spheres[j] - spheres[i]) / dist
  float bx, by, bz;                    // spheres[j].xyz
  float cos_lit;                       // dot(-tolightnorm, u) <= cos_lit => factor 1 (or -2)
};

struct GlslMat {                       // per uniform index: uvs[k], lights[k], spheres[k].xyz
  float uv[4];
  float light[4];
  float cx, cy, cz, pad;
};

struct GlslFrame {
  float campos[3];
  float fwd[3], right[3], up[3];
  float fov_x, fov_y, hk, vk;          // hk = fov.x / size.x * 2 (:172), vk likewise
  int32_t sc, lc, all;
  int32_t cam_negzero;                 // a campos component is -0.0 (wall pass, below)
  int32_t wall_start;                  // first wall-pass iteration that can change a lane
  // The per-wave wall cull's distance margin (glsl_trace.hip wall_mask): 1e-3 of the largest
  // coordinate the wall pass can reach, + 1e-4; 0 disables the cull (a -0.0 in campos, more than
  // 64 walls, non-finite bounds)
  float wall_cull_margin;
  int32_t width, height, row0, rows, tiles_x;
  const GlslWall* walls;
  const GlslBall* balls;               // all - sc entries (lights, then ospheres)
  const GlslPair* pairs;               // [light][shadow ball], lc x (all - sc - lc)
  const GlslMat* mats;                 // kGlslMax entries
  const uint32_t* mip;                 // RGBA8 levels back to back
  int32_t mip_levels;
  int32_t mip_w[kGlslMipLevels], mip_h[kGlslMipLevels], mip_off[kGlslMipLevels];
  long long out_pitch;                 // in pixels
  uint32_t* out;
  int* status;                         // bit 0: march cap reached
  // Adaptive tile order (sfrt_sched.h): 8x8 tiles, one per one-wave
  // workgroup, slot -> tile_order; cost = the tile's longest metaball march.
  const uint32_t* tile_order;
  uint8_t* tile_cost;
  const uint8_t* prev_cost;
  uint32_t* next_order;
  // tile_order's classes are the ones in tile_cost: store only changed classes (sfrt_device.h
  // store_cost, sfrt_sched.h TileSchedPtrs::cost_diff)
  int32_t cost_diff;
  // SFRT_OPT_SUPERSAMPLE: log2 of the factor S (0, 1, 2).  Read by the host only (launch_glsl
  // picks the kernel, glsl_tile_key carries it).  When > 0 the frame is the S * width x S * height
  // render target: width / height / row0 / rows / tiles_x / hk / vk are of the sample grid, out
  // and out_pitch in output pixels (glsl_trace.hip fragment).
  int32_t ss;
};

// The per-pixel planes of sfrt_glsl_draw_aux / sfrt_glsl_draw_image_aux: device
// pointers, null = not wanted, pitches in elements.  A kernel argument of its own behind the
// frame record: the plain kernels' arguments stay what they were.  Addressed as f.out is, in
// output pixels relative to row0.
struct GlslAux {
  float* depth;                        // totalDist after rayShader.frag:117
  int32_t* sphere;                     // drawSphere after :118
  int32_t* steps;                      // trips of the metaball loop :94-112
  long long depth_pitch, sphere_pitch, steps_pitch;
};

// A batch of caller-supplied rays (sfrt_glsl_cast_rays[_device]): ray q's direction
// at dirs + 3 q, un-normalised, every ray from f.campos.  Outputs null = not wanted, at least one.
struct GlslRays {
  const float* dirs;
  long long count;
  float* pos;                          // 3 floats per ray: pos after :119
  float* depth;
  int32_t* sphere;                     // -1: invalid ray
  int32_t* steps;
  uint32_t* rgba;
};

// A batch of camera views in one launch (sfrt_glsl_render_views[_aux]): view k's
// record at dev_views[k], the per-camera part of a GlslFrame under the frame's own field names --
// what sfrt_glsl.cpp's camera_terms derives from campos, rotation and fov (and `size`) -- with the
// view's target and, for the plane-writing kernels, its planes.  Everything else (the counts, the
// tables, the ground, the size, the pitch, the status word) is the launch's one GlslFrame.
struct GlslViewRec {
  float campos[3];
  float fwd[3], right[3], up[3];
  float fov_x, fov_y, hk, vk;
  int32_t cam_negzero;
  int32_t wall_start;
  float wall_cull_margin;
  int32_t pad;
  uint32_t* out;
  GlslAux aux;                         // all null for the plain kernels
};
static_assert(sizeof(GlslViewRec) == 136, "the host's table layout (sfrt_glsl.cpp)");

// Tile grid of the ordered GLSL kernel for f: key (> 0) and tile count.
long long glsl_tile_key(const GlslFrame& f, long long* tiles);
// done_event (hipEvent_t, may be null): recorded by the launch's own completion (its stop event).
// aux (may be null): the plane-writing kernels on the same grid; not all of its planes null.
int launch_glsl(const GlslFrame& f, void* stream, void* done_event = nullptr,
                const GlslAux* aux = nullptr);
// One wave per 64 consecutive rays (k_glsl_cast_rays).  Of f it reads campos, the counts, the
// wall pass's host terms (cam_negzero, wall_start, wall_cull_margin), the tables and the status
// word; the ground's mip chain only when rays.rgba is set.  rays.count in [1, 2^31).
int launch_glsl_rays(const GlslFrame& f, const GlslRays& rays, void* stream, void* done_event = nullptr);
// Whether `count` views of f's whole frame (row0 0, rows = height) fit one launch: at most
// 2^26 - 1 tiles a view (x) and 2^31 - 1 over all views, as the other two renderers' batches.
bool glsl_views_grid_ok(const GlslFrame& f, int count);
// One launch for `count` views of the frame f describes (no tile order): workgroup (x, y) is tile
// x, row-major, of view y.  Of f the per-camera fields and out are not read; dev_views: the table,
// staged earlier on the same stream; aux: the plane-writing kernels, every record's planes not
// all null.
int launch_glsl_views(const GlslFrame& f, const GlslViewRec* dev_views, int count, bool aux,
                      void* stream, void* done_event = nullptr);

}  // namespace sfrt
