// voxel_trace.h -- launch records shared by the voxel World host mirror
// (sfrt_voxel.cpp) and its gfx950 kernel (voxel_trace.hip).  SURVEY 8f f2.
//
// Per-frame terms the reference recomputes per pixel with libm are computed
// once on the host with the same expressions (World.cpp:62-87): per column
// i the ray's x/z direction (sinf, cosf, the edge-distortion divide) and
// atan2f(dir.z, dir.x) of VAngleXZ; per row j dir.y and r->yscale; per
// dynamic object its VNormalizeXZ'd direction's atan2f.  The kernel needs no
// transcendental.
#pragma once

#include <stdint.h>

namespace sfrt {

constexpr int kVoxSlots = 10;              // textures / dynTextures / colors (World.h:90-92)
constexpr int16_t kVoxEmpty = -32768;
// Block grid limits (sfrt_voxel_set_blocks refuses larger grids): the reference's map key
// (x << 20) + (y << 10) + z (World.cpp:385) addresses x < 2048, y, z < 1024 without overlap.
constexpr int kVoxMaxX = 2048, kVoxMaxY = 1024, kVoxMaxZ = 1024;
// On the device the world is the key-indexed byte array of cell_hit (voxel_trace.hip): byte
// (x << 20) + (y << 10) + z holds id + kVoxCellBias for a block (ids are in (-kVoxSlots,
// kVoxSlots)), 0 for no block; nx << 20 bytes, at most 2 GiB, so the buffer range fits an int.
constexpr int kVoxCellBias = 10;
static_assert(kVoxMaxY == 1024 && kVoxMaxZ == 1024, "the key's y and z fields are 10 bits");
static_assert((long long)kVoxMaxX << 20 <= (1ll << 31), "byte offsets and the range fit 31 bits");
static_assert(2 * (kVoxSlots - 1) + 1 <= 255, "a code fits a byte");

struct VoxDyn {                             // struct Dynamic fields Raycast reads (World.h:25-38)
  float px, py, pz;
  float sx, sy;                             // size
  float r, g, b;
  float dist;                               // distToCamera
  float atan_b;                             // atan2f of VNormalizeXZ(pos - cam.pos) (World.cpp:361)
  int32_t tex;
  int32_t pad;
};

struct VoxLight {                           // struct Light (World.h:40-47)
  float px, py, pz;
  // Squared distances dd >= dd_pass have intensity / dd - dd * 0.002f <= 0 in binary32
  // (World.cpp:425-426: the light adds nothing there): dd_pass is the smallest such float, found
  // on the host by bisection over the bit patterns (the test is monotone in dd; 0 when no dd
  // passes).  The kernel's per-wave skip tests the fma-evaluated squared distance, within
  // 6 ulp (relative 2^-20) of the reference's, against dd_skip = RU(dd_pass / (1 - 2^-20)):
  // ddf >= dd_skip implies dd >= dd_pass.  Beside the position, so that the skip test's four
  // dwords are one scalar load.
  float dd_skip;
  float intensity, r, g, b;
  int32_t shadows;
};

struct VoxTex {
  const uint32_t* texels;                   // RGBA8
  int32_t w, h;
};

struct VoxFrame {
  float cam[3];
  float view_distance, shadow_distance;
  uint32_t maxiter;                         // (unsigned)(viewDistance * 1.5f), World.cpp:322
  int32_t xstart, xadd, ystart, yadd;
  int32_t sub_w, sub_row0, sub_rows;
  const float* col;                         // per column i: dir.x, dir.z, atan2f(dir.z, dir.x)
  const float* row;                         // per row j: dir.y, yscale
  const uint8_t* cells;                     // key-indexed codes (cell_hit), nx << 20 bytes
  uint32_t cell_bytes;                      // nx << 20: the buffer range
  // The fast primary DDA's bound (sfrt_voxel.cpp dda_qlim): a ray whose direction
  // has max|d_k| <= dda_qlim * min|d_k| keeps every DDA position below 2^30 in magnitude, where
  // a plain v_cvt_i32_f32 equals to_i32; 0 sends every wave to the guarded DDA
  float dda_qlim;
  VoxTex tex[kVoxSlots];
  VoxTex dyn_tex[kVoxSlots];
  uint32_t colors[kVoxSlots];               // RGBA8 packed
  const VoxDyn* dyn;
  int32_t ndyn;
  const VoxLight* lights;
  int32_t nlights;
  long long out_pitch;
  uint32_t* out;
  int* status;                              // bit 1: out-of-range texel read
  // Adaptive tile order (sfrt_sched.h): one 8x8 tile per one-wave
  // workgroup, slot -> tile_order; cost = the tile's DDA + shadow-ray steps.
  const uint32_t* tile_order;
  uint8_t* tile_cost;
  const uint8_t* prev_cost;
  uint32_t* next_order;
  // tile_order's classes are the ones in tile_cost: store only changed classes (sfrt_device.h
  // store_cost, sfrt_sched.h TileSchedPtrs::cost_diff)
  int32_t cost_diff;
  // SFRT_OPT_SUPERSAMPLE: log2 of the factor S (0, 1, 2).  Read by the host only (launch_voxel
  // picks the kernel, voxel_tile_key carries it).  When > 0 the frame is the S * width x S * height
  // sample frame: xstart / xadd / ystart / yadd / sub_w / sub_row0 / sub_rows and the col / row
  // tables are in samples, out and out_pitch in output pixels (voxel_trace.hip voxel_tile).
  int32_t ss;
};

// The optional per-pixel planes of the frame fill (sfrt_voxel_render_band_aux):
// device pointers, null = not wanted, pitches in elements (dwords).  Row r, column a of the band
// (output pixels) at plane[r * pitch + a].  A kernel argument of its own, so that VoxFrame and
// with it every plain kernel's scalar loads stay as they are.
struct VoxAux {
  float* depth;
  int32_t* cell;
  int32_t* face;
  int32_t* steps;
  long long depth_pitch, cell_pitch, face_pitch, steps_pitch;
};

// Tile grid of launch_voxel for f (8x8 tiles, of samples when f.ss > 0): key (> 0) and tile count.
long long voxel_tile_key(const VoxFrame& f, long long* tiles);
// done_event (hipEvent_t, may be null): recorded by the launch's own completion (its stop event).
// aux != nullptr (at least one plane set): the plane-writing kernels on the same grid.
// place_xstride > 0 (sfrt_voxel_render_subset): the placing kernels -- the subset stored in place
// in a whole frame, output column a at element a * place_xstride of its row, f.out the subset's
// first pixel and f.out_pitch (and aux's pitches) the elements between two subset rows; row-major,
// f linked into no tile-order chain, with or without aux.
int launch_voxel(const VoxFrame& f, void* stream, void* done_event = nullptr,
                 const VoxAux* aux = nullptr, int place_xstride = 0);

// A batch of camera views in one launch (sfrt_voxel_render_views[_aux]): view k's
// record at dev_views[k], the per-camera part of a VoxFrame -- what sfrt_voxel.cpp's col_table,
// row_table, dyn_table and dda_qlim derive from the camera (and, with SFRT_VOXEL_VIEWS_DYNAMICS,
// from the view's own list order) -- with
// the view's target and, for the aux call, its planes (pitches in elements).  Read by the kernel
// through the constant address space, a dword at a time: a multiple of 4 bytes, 8-byte aligned.
struct VoxViewRec {
  float cam[3];
  float dda_qlim;
  const float* col;
  const float* row;
  const VoxDyn* dyn;                        // the frame's ndyn records, this view's atan_b (and order)
  uint32_t* out;                            // rows f.out_pitch apart
  VoxAux aux;
  // a view is row-major and in no tile-order chain: constants where a frame has pointers, so the
  // kernel's sorter and order lookup fold away (voxel_trace.hip voxel_tile)
  static constexpr const uint32_t* tile_order = nullptr;
  static constexpr const uint8_t* prev_cost = nullptr;
};
static_assert(sizeof(VoxViewRec) == 112, "the host's table layout (sfrt_voxel.cpp)");
// Whether `count` views of f's whole frame fit one launch: at most 2^26 - 1 tiles a view (x) and
// 2^31 - 1 workgroups in all.
bool voxel_views_grid_ok(const VoxFrame& f, int count);
// One launch for `count` views of the frame f describes (sub_row0 0, no tile order): grid
// (tiles, count), workgroup (x, y) tile x, row-major, of view y.  Of f it takes everything but
// cam, dda_qlim, col, row, dyn and out, which each view's record supplies; aux: the records'
// planes are written (every record has at least one).  done_event as launch_voxel's.
int launch_voxel_views(const VoxFrame& f, const VoxViewRec* dev_views, int count, bool aux,
                       void* stream, void* done_event = nullptr);

// A batch of caller-supplied rays (sfrt_voxel_cast_rays[_device]): device pointers,
// ray q's direction at dirs[3q..3q+2] (r->dir verbatim), its r->yscale at yscales[q] (null: 1.0f
// for every ray), its origin at origins[3q..3q+2] (null: f.cam, with the billboards); every
// output one element per ray (pos 3 floats, rgba one packed dword) or null, not all null.
struct VoxRays {
  const float* dirs;
  const float* yscales;
  const float* origins;
  long long count;
  float* pos;
  float* depth;
  int32_t* cell;
  int32_t* face;
  int32_t* steps;
  uint32_t* rgba;
};
// One wave per 64 consecutive rays (k_voxel_cast_rays).  Of f it reads the camera, the view and
// shadow distances, maxiter, the grid, the textures, colours, billboards and lights and the
// status word: no frame tables, no subset, no output, no tile order.  done_event as launch_voxel's.
int launch_voxel_rays(const VoxFrame& f, const VoxRays& rays, void* stream, void* done_event = nullptr);

// sfrt_voxel_cast_shadow_rays[_device]'s bound on max_dist (SFRT_VOXEL_MAX_SHADOW_DIST): the
// reference's trip limit is max(maxDist * 2, 20), so this is at most 8192 trips per ray.
constexpr float kVoxMaxShadowDist = 4096.0f;
// A batch of World::LRaycast queries: r->pos, r->dir (verbatim) and r->maxDist per ray; free_
// (1 free, 0 blocked or out of trips, -1 invalid) and steps (trips of the loop's body), either
// null but not both.  Of f it reads the grid alone (k_voxel_shadow_rays).
struct VoxShadowRays {
  const float* origins;
  const float* dirs;
  const float* max_dists;
  long long count;
  int32_t* free_;
  int32_t* steps;
};
int launch_voxel_shadow_rays(const VoxFrame& f, const VoxShadowRays& rays, void* stream,
                             void* done_event = nullptr);

// Rewrites the key-indexed grid `cells` for a world of nx x ny x nz codes (`codes`, device,
// x-major then y then z, as set_blocks takes them): every byte of planes x < bx, rows y < by,
// columns z < bz gets its code inside the world and 0 outside it.  (bx, by, bz) covers the world
// and every byte an earlier world may have left non-zero, so the grid is the new world's alone.
int launch_voxel_cells(uint8_t* cells, const uint8_t* codes, int nx, int ny, int nz, int bx, int by,
                       int bz, void* stream);

}  // namespace sfrt
