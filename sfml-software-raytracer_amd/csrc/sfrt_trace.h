// sfrt_trace.h -- per-frame launch record shared by the host mirror
// (sfrt_world.cpp) and the gfx950 kernels (sphere_trace.hip).
//
// Everything that the reference recomputes per pixel but is uniform over the
// frame is computed once on the host with the reference's own expressions
// (camera basis SphereWorld.cpp:100-104, ray-angle steps :85-89, the first
// march iteration from cam.pos, per-sphere atan2f(c.z, c.x) of :326) and
// shipped here, so the kernel only does per-pixel work.
#pragma once

#include <stdint.h>

namespace sfrt {

constexpr int kInlineSpheres = 64;    // spheres carried in the kernel-argument segment
constexpr int kMaxSpheres = 1024;     // 16 culling words of 64 spheres, compacted per wave
constexpr int kTile = 8;              // tile rows; a wave's tile is (8R) x 8 pixels
constexpr int kMaxIterations = 1 << 20;  // march guard; the reference has none
// Per-wave culling is proven safe while every lane of the wave has made at
// most this many march steps (the accumulated binary32 error of the march
// positions stays below the culling margin, see cull_margin); a wave that
// goes further switches to the full sphere list for the rest of its march.
constexpr int kCullSafeIterations = 1024;
constexpr int kPairMinSpheres = 16;  // above this, n <= 64 frames use 16x8 tiles (2 px per lane)
#ifndef SFRT_SLOTS
#define SFRT_SLOTS 2
#endif
// -DSFRT_EXP=<bits>: a diagnostic build (sfrt_probe.h; wrong bytes by design), said once for the
// kernels and the host: such a build never reads the hit cache, it exists to time the march.
#ifndef SFRT_EXP
#define SFRT_EXP 0
#endif
constexpr bool kDiagnosticBuild = SFRT_EXP != 0;
constexpr int kSlots = SFRT_SLOTS;  // culled spheres held in SGPRs per wave (2: best of 0-4, 6; profiles/ab/r2_ab32)

// One sphere as the kernel reads it: 32 B, one s_load_dwordx8.
struct SphereRec {
  float cx, cy, cz, r;
  float s_pass;    // exact pass threshold: r - sqrtf(s) > 0.01f  <=>  s < s_pass
  float atan_c;    // atan2f(cz, cx), the centre term of VAngleXZ (SphereWorld.cpp:326)
  uint32_t tex_off;  // this sphere's texture (textures[0], or its extension slot) in the atlas
  uint32_t tex_wh;   // its width | height << 16
};

struct FrameRec {
  float cam[3];
  float fwd[3], right[3], up[3];   // basis after VRotateX/VRotateY (SphereWorld.cpp:100-104)
  float h_start, h_inc, v_start, v_inc;  // SphereWorld.cpp:85-89
  float first_l;                    // largestDist of the first march iteration (pos == cam)
  int first_draw;                   // drawSphere after the first iteration
  int n;                            // sphere count
  int width, height;                // global frame (bounds for the subset walk)
  int xstart, xadd, ystart, yadd;   // UpdateImage pixel subset (SphereWorld.cpp:94,97)
  int sub_w;                        // columns in the subset
  int sub_row0, sub_rows;           // subset rows rendered by this launch
  // Supersampled (ss > 0, below): h_inc / v_inc are those of the S*width x S*height sample
  // frame, the subset is counted in samples (S per addressed output pixel, so sub_w, sub_row0
  // and sub_rows are multiples of S), xstart / xadd / ystart / yadd are S times the caller's,
  // and compact sample a is frame sample xstart + (a / S) * xadd + a % S (rows likewise).
  int tiles_x;                      // ceil(sub_w / 8)
  int cull;                         // 1: per-wave cone culling (default), 0: every sphere
  float cull_margin;                // absolute inflation of every sphere in the cone test
  int rays;                         // SFRT_OPT_RAYS_PER_LANE: 0 = the kernel table's choice, 1-4 forced
  long long out_pitch;              // output pitch in pixels
  uint32_t* out;                    // pixel (a, b) -> out[(b - sub_row0) * out_pitch + a]
                                    // (ss > 0: out[((b - sub_row0) >> ss) * out_pitch + (a >> ss)])
  const uint32_t* tex;              // RGBA8 texture atlas (every loaded slot, back to back)
  const SphereRec* spheres;         // device copy (used when n > kInlineSpheres)
  int* status;                      // device word: bit 0 = march guard hit, bit 1 = bad texel
  // Adaptive tile order ("Tile order"), one-wave-per-workgroup
  // kernels only; all null = row-major order, nothing recorded.  Launch k of a
  // chain (stream-ordered launches with one tile grid) dispatches tile slot s on
  // tile tile_order[s] (longest tiles of launch k-2 first) and records each
  // tile's march-step class (tile_bucket) in tile_cost.  With prev_cost set the
  // grid has one extra workgroup, 0, dispatched first: it sorts launch k-1's
  // classes into next_order for launch k+1 (stable counting sort in its LDS, no
  // atomics) and renders nothing; tile slot s is then workgroup s + 1.
  const uint32_t* tile_order;
  uint8_t* tile_cost;
  const uint8_t* prev_cost;
  uint32_t* next_order;
  // The camera moved since the launch whose classes the sorter ranks: rank each
  // tile by the longest of it and its row neighbours (sfrt_device.h sort_tiles).
  int order_dilate;
  // tile_order's classes are the ones in tile_cost: store only changed classes (sfrt_device.h
  // store_cost, sfrt_sched.h TileSchedPtrs::cost_diff)
  int32_t cost_diff;
  // SFRT_OPT_SUPERSAMPLE: log2 of the factor S (0, 1, 2).  Read by the host only (launch_trace
  // picks the kernel instantiated for it, trace_tile_key carries it); the kernels take it as a
  // template argument.
  int32_t ss;
};

// Kernel argument for n <= kInlineSpheres: frame + spheres in the kernarg segment.
struct InlineArgs {
  FrameRec f;
  SphereRec s[kInlineSpheres];
};

struct TileRec;      // sfrt_raycache.h
struct CullRec;      // sfrt_raycache.h
struct TraceCaches;  // sfrt_raycache.h

struct PixelDump {
  float pos[3];
  int draw;
  int iters;  // loop trips of SphereWorld.cpp:362 (the host's first one included)
  float xcoord, ycoord, brightness;
  uint32_t texel[2];
  uint32_t rgba;
};

// Float intermediates out of the frame-fill kernels themselves (sfrt_world_trace_points):
// the DUMP instantiation of the same march and shading, plus an epilogue that writes
// pixel (a, b)'s record to out[q] when pix[q] == (b - sub_row0) * sub_w + a (binary search
// of the sorted, distinct listed pixels: O(listed pixels) memory whatever the frame size).
// The DUMP kernels store no frame pixel (each record carries its rgba).
struct DumpArgs {
  const int64_t* pix;  // ascending, distinct
  int npix;
  PixelDump* out;      // npix records
};

// The optional per-pixel planes of the frame fill (sfrt_world_render_band_aux),
// written by the AUX instantiation of the same march and shading beside the colour: 4 bytes
// per output pixel each, addressed like the colour -- pixel (a, b) at
// plane + ((b - sub_row0) >> ss) * pitch + (a >> ss) (pitches in elements) --, a null plane
// is not written.  Supersampled, the output pixel's first sample (its group's leader lane).
// A kernel argument of its own, as DumpArgs is: FrameRec's layout is every kernel's.
struct AuxArgs {
  float* depth;        // |pos - cam| of the hit (shade_texel's bl, before max(.., 3.0f))
  int32_t* sphere;     // drawSphere
  int32_t* steps;      // loop trips of SphereWorld.cpp:362 (the host's first one included)
  long long depth_pitch, sphere_pitch, steps_pitch;
};

// A batch of caller-supplied rays (sfrt_world_cast_rays[_device]): ray q's
// direction is dirs[3q..3q+2] (un-normalised, as Raycast receives r->dir), its origin
// origins[3q..3q+2], or f.cam for every ray when origins is null.  One element per ray in every
// non-null output (pos: three floats).  A kernel argument of its own, as DumpArgs and AuxArgs
// are: FrameRec's layout is every kernel's.
struct RayArgs {
  const float* dirs;
  const float* origins;
  long long count;
  float* pos;        // r->pos after the march
  float* depth;      // |pos - origin| (:375's VLength, before its std::max)
  int32_t* sphere;   // drawSphere; -1: invalid ray
  int32_t* steps;    // loop trips of :362, the first one included; 0: invalid ray
  uint32_t* rgba;    // r->c of :373-381
};

// The ray-batch kernels (k_cast_rays): one wave per 64 consecutive rays, one ray per lane.  Of
// f they read cam, first_l, first_draw, n, cull, cull_margin, tex, spheres and status; the
// frame and tile-order members are ignored.  done_event as for launch_trace.
int launch_cast_rays(const FrameRec& f, const SphereRec* host_spheres, const RayArgs& rays,
                     void* stream, void* done_event);

// sphere_trace.hip.  dump != nullptr: the DUMP instantiation of the kernel the table picks.
// aux != nullptr (with at least one plane set): its AUX instantiation -- never with dump or
// the ray cache.
// place_xstride > 0 (sfrt_world_render_subset): the placing kernels -- the subset stored in place
// in a whole frame, compact column a at element (a >> ss) * place_xstride of its row, f.out the
// subset's first pixel and f.out_pitch (and aux's pitches) the elements between two subset rows;
// a row-major launch only (no tile order, no ray cache, no dump), with or without aux.
// done_event (hipEvent_t, may be null): recorded by the list kernel's own completion (its stop
// event; the inline kernel, which reads no device records, takes none).
// caches (may be null: today's kernel): what the chain's caches decided for this launch
// (sfrt_raycache.h ChainCaches::begin), every buffer filled for this very f and these very records
// earlier on the same stream.  Each layer needs the one before it -- dirs with tile_recs (an
// ordered, non-dump launch only): the directions, the tiles' culling cones and grid positions are
// loaded; cull_recs with cull_wins: so are each tile's culling mask and march windows, and no
// tile record is read; hit_recs with hit == kFill: the cull-cached launch also stores each ray's
// march result; with hit == kRead: no march -- one wave per tile in tile-number order shades from
// the records.  That launch takes no part in the tile order: f's tile_order, tile_cost, prev_cost
// and next_order are ignored (the caller links nothing), and dirs and cull_wins are not read.
// texel_recs and compact_recs ride on such a launch in the same way: kFill, it also stores them;
// kRead, it shades from them (compact: with bright_rep, the world's class table, never with ss > 0).
// pixels rides on a launch that reads the texel records: kFill, that launch raises its status bits in
// pixel_status in place of f.status and its band is then copied into pixels (k_pixels_copy), which
// also ORs that word into f.status; kRead, the launch is that copy out of pixels and nothing else.
int launch_trace(const FrameRec& f, const SphereRec* host_spheres, void* stream,
                 const DumpArgs* dump = nullptr, void* done_event = nullptr,
                 const TraceCaches* caches = nullptr, const AuxArgs* aux = nullptr,
                 int place_xstride = 0);
// Whether k_pixels_copy can address f's band of output pixels (its units fit the grid): a launch
// that cannot takes no part in the pixel layer.
bool pixel_copy_fits(const FrameRec& f);
// Fills ray_cache (ray_cache_bytes(tiles, rays) bytes, sfrt_raycache.h, of the grid
// trace_tile_key names) with the primary directions of f's rays, tile-major, and tile_recs
// (tile_rec_bytes(tiles) bytes) with the tiles' records.
int launch_ray_fill(const FrameRec& f, float* ray_cache, TileRec* tile_recs, void* stream);
// Fills cull_recs (cull_rec_bytes(tiles) bytes, sfrt_raycache.h) and cull_wins
// (cull_win_bytes(tiles, f.n > kInlineSpheres) bytes) of the same grid with what each tile's wave
// of launch_trace(f, host_spheres, ...) would cull, from the cones in tile_recs (filled for f
// earlier on the same stream).  n > kInlineSpheres: the records are read from f.spheres.
int launch_cull_fill(const FrameRec& f, const SphereRec* host_spheres, const TileRec* tile_recs,
                     CullRec* cull_recs, void* cull_wins, void* stream);
// A batch of camera views in one launch (sfrt_world_render_views[_aux]): view k's
// record in a device table, the frame exactly as render_band's launch of a whole frame would
// carry it in its arguments (f.spheres: the view's records in the same table, at least
// kInlineSpheres of them readable; tile_order, tile_cost, prev_cost and next_order unused) and
// its planes (read by the aux kernels only).
struct ViewRec {
  FrameRec f;
  AuxArgs a;
};
// The tile grid of one view of the batch: pixels per lane by the row-major kernel table (f.rays
// overrides it), the tiles of a row (the f.tiles_x of every record) and of a whole view.
void trace_views_grid(const FrameRec& f, int* tiles_x, long long* tiles);
// One launch for count views of one size: workgroup (x, y) is tile x, row-major, of view y, so the
// views run in table order.  f: any view's record (its size, n, ss and rays choose the kernel);
// dev_views: the table, staged earlier on the same stream; aux: the plane-writing kernels.
// done_event (may be null): the launch's stop event, as launch_trace's.
int launch_trace_views(const FrameRec& f, const ViewRec* dev_views, int count, bool aux,
                       void* stream, void* done_event);
// "release" for the shipped build; "diagnostic" (-DSFRT_EXP: wrong bytes by design) or
// "ab" (EXTRA build flags, tools/ab_libs.py) otherwise.
const char* trace_build_flavour();
// Tile grid of the kernel launch_trace picks for f when that kernel takes part in
// the adaptive tile order: a key naming the grid (> 0) and its tile count; else 0.
// Bits 0-27 tiles_y, 28-55 tiles_x, 56-58 pixels per lane, 59-60 f.ss.
long long trace_tile_key(const FrameRec& f, long long* tiles);
// An upper bound of the workgroups launch_trace would launch for f in either tile order, so
// that a caller can refuse a grid it cannot launch (> 0x7fffffff) before queuing anything.
long long trace_blocks(const FrameRec& f);

}  // namespace sfrt
