// sfrt_voxel.cpp -- host side of the voxel World frame fill:
// a C++ mirror of the state World::UpdateImage reads and the extern "C"
// entry points sfrt_voxel_* of include/sfrt.h.
//
// Reference (paths under /root/reference/Raytracing/):
//   class World                     World.h:58-97 (width/height 320x180, shadowDistance 16,
//                                   viewDistance 24, Camera defaults World.h:9-19)
//   World::World (fov -> radians)   World.cpp:55-56
//   World::UpdateImage              World.cpp:62-87 (per-column / per-row terms below)
//   blocks, textures, dynTextures,  World.h:75, 90-95
//   colors, dyn, alights
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <algorithm>
#include <vector>

#include "sfrt.h"
#include "sfrt_host.h"
#include "sfrt_sched.h"
#include "sfrt_math.h"
#include "voxel_trace.h"

#pragma clang fp contract(off)

namespace {

constexpr float kPI = 3.1415926535f;  // World.h:5

// The light's contribution test of World::Raycast, `intensity / dd - dd * 0.002f > 0`
// (World.cpp:425-426), for a squared distance dd >= 0: true for dd below a threshold and false
// from it on (intensity / dd never increases with dd, dd * 0.002f never decreases, and each
// rounds monotonically), so the smallest non-negative float where it is false is found by
// bisection over the bit patterns of [+0, +inf].  The kernel skips a light for a wave none of
// whose lanes has dd below it (VoxLight::dd_skip).
static bool light_adds(float intensity, float dd) {
  volatile float q = intensity / dd;   // binary32, correctly rounded (no contraction: FLAGS)
  volatile float p = dd * 0.002f;
  return q - p > 0.0f;
}
float light_dd_pass(float intensity) {
  uint32_t lo = 0u, hi = 0x7f800000u;  // light_adds(+inf) is false for every intensity
  if (!light_adds(intensity, 0.0f)) return 0.0f;
  while (hi - lo > 1u) {               // invariant: adds at lo, not at hi
    const uint32_t mid = lo + (hi - lo) / 2u;
    float m;
    std::memcpy(&m, &mid, 4);
    if (light_adds(intensity, m)) lo = mid; else hi = mid;
  }
  float t;
  std::memcpy(&t, &hi, 4);
  return t;
}

// VoxLight::dd_skip from dd_pass: RU(dd_pass / (1 - 2^-20)), so that a squared distance
// evaluated with fmas (relative error within 2^-20 of the reference's three products and two
// sums, all terms non-negative) at or above it implies the reference's dd >= dd_pass.
float light_dd_skip(float dd_pass) {
  const double t = (double)dd_pass / (1.0 - 0x1.0p-20);
  const float f = (float)t;
  return (double)f >= t ? f : std::nextafter(f, INFINITY);
}

// The fast primary DDA's bound (VoxFrame::dda_qlim, voxel_trace.hip pos_i32).  At a position
// with |p| < 2^30, a step of World::Raycast (World.cpp:330-350) divides a numerator in (-1, 2)
// (dirXadd + sign * (p - (int)p)) by |d_k|, so |raySpeed| <= 2 (1 + 2^-23) / m with
// m = min_k |d_k| (a negative fraction can make it negative), and moves axis j by at most
// |d_j| (|raySpeed| + 0.002)(1 + 2^-21) <= 2.0001 X / m + 0.0021 X (X = max_k |d_k| <= xmax),
// plus the add's rounding, <= 32 below 2^30.  So with Q = X / m, S = 2.001 Q + 0.003 xmax + 33
// bounds one step and |cam| + (maxiter + 1) S <= 2^30 keeps every position of the walk below
// 2^30, where the plain conversion equals to_i32 (only +2^31 and beyond and NaN differ).  The
// kernel takes the fast DDA for a wave whose every lane has X <= qlim * m (the float product
// rounds up at most 2^-24, absorbed by rounding qlim down by 2^-20); 0 disables it.
float dda_qlim(const float cam[3], uint32_t maxiter, float xmax) {
  const double p = std::max({std::fabs((double)cam[0]), std::fabs((double)cam[1]),
                             std::fabs((double)cam[2])});
  const double q = ((1073741824.0 - p) / ((double)maxiter + 1.0) - 33.0 - 0.003 * xmax) / 2.001;
  if (!(q > 1.0) || !std::isfinite(xmax)) return 0.0f;
  const float f = (float)(q * (1.0 - 0x1.0p-20));
  return (double)f <= q * (1.0 - 0x1.0p-20) ? f : std::nextafter(f, 0.0f);
}

// float -> unsigned as the reference's x86-64 build converts it.
uint32_t to_u32(float f) {
  if (!(f > -9.2233720368547758e18f && f < 9.2233720368547758e18f)) return 0u;
  return (uint32_t)(int64_t)f;
}

struct DevTex {
  uint32_t* d = nullptr;
  int w = 0, h = 0;
  size_t cap = 0;
};

// The per-camera tables of a frame (World.cpp:64-87 at the sample size W x H), each into the
// caller's block: the band path (sfrt_voxel::prepare) builds them for the world's camera, a view
// batch (render_views_body) once per view.  col_table and row_table return the largest finite
// |component| they wrote (dda_qlim's xmax is the larger of the two).
float col_table(const sfrt_camera& cam, int W, float* col) {
  const float hStart = cam.rotation - cam.fov_h / 2;
  const float hIncreaseBy = cam.fov_h / W;
  float xmax = 0.0f;
  for (int i = 0; i < W; i++) {
    const float hray = (hStart + hIncreaseBy * i);
    const float fix = std::cos(cam.rotation - hray);
    const float dx = std::sin(hray) / fix, dz = std::cos(hray) / fix;
    col[3 * (size_t)i] = dx;
    col[3 * (size_t)i + 1] = dz;
    col[3 * (size_t)i + 2] = sfrt_math::atan2f(dz, dx);  // VAngleXZ's ray term (World.cpp:272)
    for (float c : {dx, dz})
      if (std::isfinite(c)) xmax = std::max(xmax, std::fabs(c));
  }
  return xmax;
}
float row_table(const sfrt_camera& cam, int H, float* row) {
  const float vStart = cam.fov_v / 2;
  const float vIncreaseBy = cam.fov_v / H;
  const float vOff = std::sin(cam.hrotation);
  float xmax = 0.0f;
  for (int j = 0; j < H; j++) {
    const float vray = (vStart - j * vIncreaseBy);
    row[2 * (size_t)j] = (vOff + std::sin(vray));
    row[2 * (size_t)j + 1] = std::cos(cam.hrotation + vray);   // r->yscale
    if (std::isfinite(row[2 * (size_t)j])) xmax = std::max(xmax, std::fabs(row[2 * (size_t)j]));
  }
  return xmax;
}
// The billboards as the kernel reads them, in the order given, atan_b for this camera.
void dyn_table(const sfrt_camera& cam, const sfrt_dynamic* dyn, size_t n, sfrt::VoxDyn* vd) {
  for (size_t k = 0; k < n; k++) {
    const sfrt_dynamic& d = dyn[k];
    sfrt::VoxDyn& o = vd[k];
    o.px = d.pos[0]; o.py = d.pos[1]; o.pz = d.pos[2];
    o.sx = d.size[0]; o.sy = d.size[1];
    o.r = d.r; o.g = d.g; o.b = d.b;
    o.dist = d.dist_to_camera;
    // VNormalizeXZ(d->pos - cam.pos) (World.cpp:282-285, 361)
    const float ex = d.pos[0] - cam.pos[0], ez = d.pos[2] - cam.pos[2];
    const float l = std::sqrt(ex * ex + ez * ez);
    o.atan_b = sfrt_math::atan2f(ez / l, ex / l);
    o.tex = d.texture_id;
    o.pad = 0;
  }
}
void light_table(const sfrt_light* lights, size_t n, sfrt::VoxLight* vl) {
  for (size_t k = 0; k < n; k++) {
    const sfrt_light& L = lights[k];
    sfrt::VoxLight& o = vl[k];
    o.px = L.pos[0]; o.py = L.pos[1]; o.pz = L.pos[2];
    o.dd_skip = light_dd_skip(light_dd_pass(L.intensity));
    o.intensity = L.intensity; o.r = L.r; o.g = L.g; o.b = L.b;
    o.shadows = L.shadows;
  }
}
size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// sfrt_voxel_sort_dynamics: distToCamera of World.cpp:226-227 for every element, then the list
// ordered by insertion from the front with World.cpp:229's `<` -- element i goes before the first
// already placed element whose distance is greater (a NaN distance is greater than nothing and
// nothing is greater than it).  Stable and ascending.
void sort_dynamics(sfrt_dynamic* dyn, size_t n, const float cam_pos[3]) {
  for (size_t i = 0; i < n; i++) {
    const float tx = dyn[i].pos[0] - cam_pos[0], tz = dyn[i].pos[2] - cam_pos[2];
    dyn[i].dist_to_camera = std::sqrt(tx * tx + tz * tz);
  }
  for (size_t i = 1; i < n; i++) {
    const sfrt_dynamic e = dyn[i];
    size_t j = 0;
    while (j < i && !(e.dist_to_camera < dyn[j].dist_to_camera)) j++;
    if (j == i) continue;
    std::memmove(dyn + j + 1, dyn + j, (i - j) * sizeof(sfrt_dynamic));
    dyn[j] = e;
  }
}

bool camera_ok(const sfrt_camera& cam) {  // sfrt_voxel_set_camera's test
  for (float c : {cam.pos[0], cam.pos[1], cam.pos[2], cam.rotation, cam.hrotation, cam.fov_h, cam.fov_v})
    if (!std::isfinite(c)) return false;
  return true;
}


}  // namespace

struct sfrt_voxel {
  int device = 0;
  // --- World state read by UpdateImage ---
  int width = 320, height = 180;            // World.h:67-68
  sfrt_camera cam{};
  float shadow_distance = 16.0f;            // World.h:70
  float view_distance = 24.0f;              // World.h:71
  std::vector<int16_t> blocks;
  int nx = 0, ny = 0, nz = 0;
  uint32_t colors[sfrt::kVoxSlots] = {};
  std::vector<sfrt_dynamic> dyn;
  std::vector<sfrt_light> lights;
  // --- device resources ---
  hipStream_t stream = nullptr;
  DevTex tex[sfrt::kVoxSlots], dyn_tex[sfrt::kVoxSlots];
  sfrt::DeviceBuf d_cells;  // the key-indexed byte grid (voxel_trace.h, cell_hit)
  // Every byte of d_cells outside planes x < box[0], rows y < box[1], columns z < box[2] is 0.
  int box[3] = {0, 0, 0};
  bool blocks_dirty = true;
  // The codes of a set_blocks on their way to the grid: pinned staging, its device copy, and the
  // event after the rewrite that read them.  Two in turn, so that blocks set on consecutive frames
  // do not wait on the host for the previous rewrite (which may sit behind other work on its
  // stream); an upload reuses a pair only after that pair's previous rewrite has run.
  struct CodeStage {
    sfrt::PinnedBuf h;
    sfrt::DeviceBuf d;
    hipEvent_t ev = nullptr;
    bool pending = false;
  };
  CodeStage stage[2];
  int stage_next = 0;
  // d_cells' and the textures' rewrites ordered against their readers (sfrt_host.h)
  sfrt::SharedBuffer shared;
  sfrt::PinnedStage tex_stage;  // texture uploads from the caller's memory
  // Per-frame tables (columns | rows | dyn | lights) in a ring of slots, each
  // with pinned staging and the event of the last launch that read it, so
  // launches on different streams never see a table overwritten under them.
  // (sfrt::TableSlot, sfrt_host.h: a reuse on another stream waits for the slot's last user.)
  // The view batches (sfrt_voxel_render_views) stage their block -- view records and every view's
  // tables -- in a ring of their own, the slots past kSlots of the same array: a batch never takes
  // the band's staged tables away (cur_slot, staged_version stay valid), and every loop over
  // `slots` -- SharedBuffer::before_write's among them, so that a grid or texture rewrite waits
  // for the batches that still read the old data -- covers both rings.
  static constexpr int kSlots = 4, kViewSlots = 4;
  sfrt::TableSlot slots[kSlots + kViewSlots];
  int next_slot = 0;
  int cur_slot = -1;
  int next_view_slot = 0;
  // The tables depend only on the size, the camera, the billboards and the lights: every
  // setter of those bumps tables_version, and a launch whose tables are unchanged since the
  // last staging reuses that slot (no host recomputation, no copy).
  uint64_t tables_version = 1, staged_version = 0;
  size_t staged_off[3] = {0, 0, 0};  // byte offsets of row | dyn | lights in the staged slot
  float staged_xmax = 0.0f;          // max finite |component| of the staged ray directions
  int* d_status = nullptr;
  // The host path (update_image): the compact subset's device buffer on `stream` and, per
  // requested plane of sfrt_voxel_update_image_aux (depth, cell, face, steps), a compact device
  // plane with its pinned staging (sfrt_host.h DeviceBuf, PinnedBuf)
  sfrt::DeviceBuf d_frame, d_aux[4];
  sfrt::PinnedBuf h_aux[4];
  // Staging of sfrt_voxel_cast_rays and sfrt_voxel_cast_shadow_rays (the host calls)
  sfrt::BatchStage ray_stage;
  int tile_order_on = 0;    // SFRT_OPT_TILE_ORDER: off by default here (slower)
  // SFRT_OPT_SUPERSAMPLE: log2 of the factor S (0, 1, 2).  S > 1: the frame's samples are the
  // pixels of World::UpdateImage at S * width x S * height (prepare() builds the tables for that
  // size), box-filtered in the kernel
  int ss = 0;
  sfrt::TileChains scheds;   // adaptive tile order (sfrt_sched.h), render_band; one chain per stream
  sfrt::Relay relay;         // events recorded on callers' streams, relayed (sfrt_host.h)
  mutable std::mutex mu;

  sfrt_voxel() {
    for (auto& t : slots) t.relay = &relay;
    shared.relay = &relay;
  }

  ~sfrt_voxel() {
    sfrt::DeviceGuard g(device);
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipDeviceSynchronize();
    scheds.release();
    for (auto& t : tex) (void)hipFree(t.d);
    for (auto& t : dyn_tex) (void)hipFree(t.d);
    (void)hipDeviceSynchronize();
    d_cells.release();
    for (CodeStage& c : stage) {
      c.d.release();
      c.h.release();
      if (c.ev) (void)hipEventDestroy(c.ev);
    }
    shared.release();
    tex_stage.release();
    for (auto& t : slots) t.release();
    relay.release();
    (void)hipFree(d_status);
    d_frame.release();
    for (int q = 0; q < 4; q++) {
      d_aux[q].release();
      h_aux[q].release();
    }
    ray_stage.release();
    if (stream) (void)hipStreamDestroy(stream);
  }

  // Builds the frame record and uploads the per-frame arrays on stream s.
  // Everything the reference recomputes per pixel but that depends only on the
  // column, the row or the object is evaluated here, with its expressions.
  // The part of a frame record that does not depend on the camera (the device pointers come with
  // fill_world, once the grid is up to date).
  void begin_frame(sfrt::VoxFrame& f) const {
    std::memset(&f, 0, sizeof f);
    f.ss = ss;
    f.view_distance = view_distance;
    f.shadow_distance = shadow_distance;
    f.maxiter = to_u32(view_distance * 1.5f);                       // World.cpp:322
  }

  int prepare(sfrt::VoxFrame& f, hipStream_t s) {
    if (blocks.empty()) return SFRT_E_EMPTY;
    if (width <= 0 || height <= 0) return SFRT_E_INVALID;
    // World.cpp:64-87 is evaluated at the sample size (ints: the frame calls checked sample_grid_ok)
    const int W = width << ss, H = height << ss;
    begin_frame(f);
    f.cam[0] = cam.pos[0]; f.cam[1] = cam.pos[1]; f.cam[2] = cam.pos[2];
    if (staged_version == tables_version && cur_slot >= 0) {
      sfrt::TableSlot& t = slots[cur_slot];  // still holds this scene's tables; launched() re-marks it
      const int rc = blocks_upload(s);  // first: fill_frame reads d_cells
      if (rc != SFRT_OK) return rc;
      HIP_TRY(shared.before_read(s));
      HIP_TRY(t.use_on(s));  // staged, or last read, on another stream: wait for it
      fill_frame(f, t.d.ptr<uint8_t>(), staged_off);
      return SFRT_OK;
    }
    // one blob per launch: col | row | dyn | lights, 16-byte aligned parts, built in place in the
    // slot's pinned copy (the per-camera parts by the functions a view batch calls per view)
    const size_t b_col = up16((size_t)W * 3 * sizeof(float)), b_row = up16((size_t)H * 2 * sizeof(float)),
                 b_dyn = up16(dyn.size() * sizeof(sfrt::VoxDyn)),
                 b_lit = up16(lights.size() * sizeof(sfrt::VoxLight));
    const size_t bytes = b_col + b_row + b_dyn + b_lit + 16;
    sfrt::TableSlot& t = slots[next_slot];
    HIP_TRY(t.reclaim());
    HIP_TRY(t.grow(bytes, s));  // no wait on other streams (sfrt_host.h)
    uint8_t* h = t.h.ptr<uint8_t>();
    const float xmax = std::max(col_table(cam, W, (float*)h), row_table(cam, H, (float*)(h + b_col)));
    dyn_table(cam, dyn.data(), dyn.size(), (sfrt::VoxDyn*)(h + b_col + b_row));
    light_table(lights.data(), lights.size(), (sfrt::VoxLight*)(h + b_col + b_row + b_dyn));
    HIP_TRY(hipMemcpyAsync(t.d.ptr(), h, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(t.staged(s));
    cur_slot = next_slot;
    next_slot = (next_slot + 1) % kSlots;
    staged_version = tables_version;
    staged_xmax = xmax;
    staged_off[0] = b_col;
    staged_off[1] = b_col + b_row;
    staged_off[2] = b_col + b_row + b_dyn;
    const int rc = blocks_upload(s);  // first: fill_frame reads d_cells
    if (rc != SFRT_OK) return rc;
    HIP_TRY(shared.before_read(s));
    fill_frame(f, t.d.ptr<uint8_t>(), staged_off);
    return SFRT_OK;
  }

  // The world as the kernel reads it: byte (x << 20) + (y << 10) + z = id + kVoxCellBias of the
  // block at (x, y, z), 0 elsewhere (the reference's map key as a linear index, voxel_trace.h).
  // nx planes of 1 MiB; each plane's ny rows of nz codes land at row pitch 1024.
  // Rare (the reference fills its map once, World.cpp:5-18) but stream-ordered like every other
  // upload: the rewrite is queued on the frame's stream s behind every launch, on any stream, that
  // read the old grid (SharedBuffer::before_write: device-side waits), and launches on other
  // streams wait for it -- a frame of another world or renderer in flight is never held up.
  // It writes only the box that holds the new world or anything an earlier one left non-zero.
  int blocks_upload(hipStream_t s) {
    if (!blocks_dirty) return SFRT_OK;
    const size_t n = blocks.size();
    CodeStage& c = stage[stage_next];
    if (c.pending) {  // this pair's previous rewrite (queued by this object, two uploads ago) has run
      HIP_TRY(hipEventSynchronize(c.ev));
      c.pending = false;
    }
    HIP_TRY(shared.before_write(s, slots));
    HIP_TRY(c.h.reserve(n));
    if (c.d.bytes() < n) {  // grows to the largest world seen (the pair is not in use: above)
      size_t cap = 1;
      while (cap < n) cap <<= 1;
      HIP_TRY(c.d.reserve(cap, s));
    }
    if (!c.ev) HIP_TRY(hipEventCreateWithFlags(&c.ev, hipEventDisableTiming));
    const size_t bytes = (size_t)nx << 20;
    bool fresh = false;
    HIP_TRY(d_cells.reserve(bytes, s, &fresh));
    if (fresh) {  // a fresh grid (stream-ordered on s), all zero
      HIP_TRY(hipMemsetAsync(d_cells.ptr(), 0, bytes, s));
      box[0] = box[1] = box[2] = 0;
    }
    uint8_t* codes = c.h.ptr<uint8_t>();
    for (size_t k = 0; k < n; k++)
      codes[k] = blocks[k] == sfrt::kVoxEmpty ? 0 : (uint8_t)(blocks[k] + sfrt::kVoxCellBias);
    HIP_TRY(hipMemcpyAsync(c.d.ptr(), codes, n, hipMemcpyHostToDevice, s));
    // planes past the new nx are outside the kernel's buffer range, but a later, larger world
    // would see them: the box covers them too while they may hold codes
    const int bx = std::max(nx, box[0]), by = std::max(ny, box[1]), bz = std::max(nz, box[2]);
    if (sfrt::launch_voxel_cells(d_cells.ptr<uint8_t>(), c.d.ptr<uint8_t>(), nx, ny, nz, bx, by, bz, s))
      return SFRT_E_HIP;
    HIP_TRY(relay.record(s, c.ev));  // s may be a caller's stream
    c.pending = true;
    stage_next ^= 1;
    HIP_TRY(shared.after_write(s));
    box[0] = nx; box[1] = ny; box[2] = nz;
    blocks_dirty = false;
    return SFRT_OK;
  }

  // A texture (textures[slot] or dynTextures[slot], World.h:90-91) uploaded stream-ordered, like the
  // grid: on the object's stream behind every frame that read the old texels (SharedBuffer), a
  // larger one in a new buffer with the old one freed in that order.  Frames queued after the call
  // read the new texels; nothing waits for the device.
  int upload_texture(DevTex& t, const uint8_t* rgba, int w, int h) {
    const size_t n = (size_t)w * h;
    void* staged = nullptr;
    HIP_TRY(tex_stage.fill(rgba, n * 4, &staged));
    HIP_TRY(shared.before_write(stream, slots));
    if (t.cap < n) {
      uint32_t* d = nullptr;
      HIP_TRY(hipMallocAsync((void**)&d, n * 4, stream));
      if (t.d) HIP_TRY(hipFreeAsync(t.d, stream));
      t.d = d;
      t.cap = n;
    }
    HIP_TRY(hipMemcpyAsync(t.d, staged, n * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(tex_stage.copied(stream));
    HIP_TRY(shared.after_write(stream));
    t.w = w;
    t.h = h;
    return SFRT_OK;
  }

  // The frame record's device pointers: the staged tables at d, the grid (blocks_upload()
  // must have run: the kernel's buffer resource over d_cells has no other guard).
  void fill_frame(sfrt::VoxFrame& f, uint8_t* d, const size_t* off) {
    f.col = (const float*)d;
    f.row = (const float*)(d + off[0]);
    f.dda_qlim = dda_qlim(f.cam, f.maxiter, staged_xmax);
    f.dyn = (const sfrt::VoxDyn*)(d + off[1]);
    f.lights = (const sfrt::VoxLight*)(d + off[2]);
    fill_world(f);
  }
  // What every view of a batch shares with a band: the grid, the textures and colours, the list
  // sizes and the status word.
  void fill_world(sfrt::VoxFrame& f) const {
    f.cells = d_cells.ptr<uint8_t>();
    f.cell_bytes = (uint32_t)nx << 20;
    for (int k = 0; k < sfrt::kVoxSlots; k++) {
      f.tex[k] = {tex[k].d, tex[k].w, tex[k].h};
      f.dyn_tex[k] = {dyn_tex[k].d, dyn_tex[k].w, dyn_tex[k].h};
      f.colors[k] = colors[k];
    }
    f.ndyn = (int)dyn.size();
    f.nlights = (int)lights.size();
    f.status = d_status;
  }

  // A sub_w x sub_rows fill's sample grid (SFRT_OPT_SUPERSAMPLE) must fit the kernel's ints and
  // launch_voxel's grid; checked before anything is allocated, queued or written.
  bool sample_grid_ok(int sub_w, int sub_rows) const {
    if (width > (0x7fffffff >> ss) || height > (0x7fffffff >> ss)) return false;
    const long long tx = (((long long)sub_w << ss) + 7) / 8, ty = (((long long)sub_rows << ss) + 7) / 8;
    return !ss || tx * ty <= 0x7ffffffeLL;
  }

  // The current table slot's event, for the launch that reads it to record (its stop event), and
  // the slot marked busy once that launch is queued on s (the event also covers the launch's
  // read of the grid: SharedBuffer).
  void* launch_event() const { return slots[cur_slot].launch_event(); }
  hipError_t launched(hipStream_t s) { return slots[cur_slot].launched_with(s); }

  int read_status(hipStream_t s) {
    int st = 0;
    HIP_TRY(sfrt::read_status(d_status, s, &st));
    return (st & 2) ? SFRT_E_TEXEL : SFRT_OK;
  }
};

extern "C" {

int sfrt_voxel_create(int hip_device, sfrt_voxel** out) {
  if (!out) return SFRT_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || hip_device < 0 || hip_device >= count)
    return SFRT_E_HIP;
  sfrt_voxel* v = new sfrt_voxel();
  v->device = hip_device;
  // Camera defaults (World.h:9-19) and the constructor's fov conversion (World.cpp:55-56).
  v->cam.pos[0] = 15.5f; v->cam.pos[1] = 1.9f; v->cam.pos[2] = 15.5f;
  v->cam.fov_h = 75.0f * (kPI / 180.0f);
  v->cam.fov_v = 47.0f * (kPI / 180.0f);
  sfrt::DeviceGuard g(hip_device);
  if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&v->d_status, sizeof(int)) != hipSuccess ||
      hipMemset(v->d_status, 0, sizeof(int)) != hipSuccess) {
    delete v;
    return SFRT_E_HIP;
  }
  *out = v;
  return SFRT_OK;
}

void sfrt_voxel_destroy(sfrt_voxel* v) { delete v; }

int sfrt_voxel_set_size(sfrt_voxel* v, int width, int height) {
  if (!v || width <= 0 || height <= 0) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  v->width = width;
  v->height = height;
  v->tables_version++;
  return SFRT_OK;
}

int sfrt_voxel_set_camera(sfrt_voxel* v, const sfrt_camera* cam) {
  if (!v || !cam) return SFRT_E_INVALID;
  if (!camera_ok(*cam)) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  v->cam = *cam;
  v->tables_version++;
  return SFRT_OK;
}

int sfrt_voxel_set_view(sfrt_voxel* v, float shadow_distance, float view_distance) {
  if (!v || !std::isfinite(shadow_distance) || !std::isfinite(view_distance) || view_distance < 0)
    return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  v->shadow_distance = shadow_distance;
  v->view_distance = view_distance;
  return SFRT_OK;
}

int sfrt_voxel_set_blocks(sfrt_voxel* v, const int16_t* texture_ids, int nx, int ny, int nz) {
  // The reference keys blocks by (x << 20) + (y << 10) + z (World.cpp:10); a
  // dense grid is exact for 0 <= x < 2048, 0 <= y, z < 1024.
  if (!v || !texture_ids || nx <= 0 || ny <= 0 || nz <= 0 || nx > sfrt::kVoxMaxX || ny > sfrt::kVoxMaxY || nz > sfrt::kVoxMaxZ)
    return SFRT_E_INVALID;
  const size_t n = (size_t)nx * ny * nz;
  for (size_t k = 0; k < n; k++)
    if (texture_ids[k] != sfrt::kVoxEmpty &&
        (texture_ids[k] >= sfrt::kVoxSlots || texture_ids[k] <= -sfrt::kVoxSlots))
      return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  v->blocks.assign(texture_ids, texture_ids + n);
  v->nx = nx; v->ny = ny; v->nz = nz;
  v->blocks_dirty = true;
  return SFRT_OK;
}

int sfrt_voxel_load_texture(sfrt_voxel* v, int slot, const uint8_t* rgba, int w, int h) {
  if (!v || !rgba || slot < 0 || slot >= sfrt::kVoxSlots || w <= 0 || h <= 0) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  sfrt::DeviceGuard g(v->device);
  return v->upload_texture(v->tex[slot], rgba, w, h);
}

int sfrt_voxel_load_dyn_texture(sfrt_voxel* v, int slot, const uint8_t* rgba, int w, int h) {
  if (!v || !rgba || slot < 0 || slot >= sfrt::kVoxSlots || w <= 0 || h <= 0) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  sfrt::DeviceGuard g(v->device);
  return v->upload_texture(v->dyn_tex[slot], rgba, w, h);
}

int sfrt_voxel_set_colors(sfrt_voxel* v, const uint8_t* rgba, int count) {
  if (!v || !rgba || count < 0 || count > sfrt::kVoxSlots) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  for (int k = 0; k < count; k++) std::memcpy(&v->colors[k], rgba + 4 * k, 4);
  return SFRT_OK;
}

int sfrt_voxel_set_dynamics(sfrt_voxel* v, const sfrt_dynamic* dyn, int count) {
  if (!v || count < 0 || (count > 0 && !dyn)) return SFRT_E_INVALID;
  for (int k = 0; k < count; k++)
    if (dyn[k].texture_id < 0 || dyn[k].texture_id >= sfrt::kVoxSlots) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  v->dyn.assign(dyn, dyn + count);
  v->tables_version++;
  return SFRT_OK;
}

float sfrt_voxel_light_dd_pass(float intensity) { return light_dd_pass(intensity); }

int sfrt_voxel_set_lights(sfrt_voxel* v, const sfrt_light* lights, int count) {
  if (!v || count < 0 || (count > 0 && !lights)) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  v->lights.assign(lights, lights + count);
  v->tables_version++;
  return SFRT_OK;
}

// sfrt_voxel_update_image and sfrt_voxel_update_image_aux (planes: depth, cell, face, steps as
// host planes of width*height elements, any null but not all; nullptr for the plain call).
static int update_image_body(sfrt_voxel* v, uint8_t* pixels, void* const* planes, int ystart,
                             int yadd, int xstart, int xadd) {
  if (!v || !pixels || ystart < 0 || xstart < 0 || yadd <= 0 || xadd <= 0) return SFRT_E_INVALID;
  if (planes && !planes[0] && !planes[1] && !planes[2] && !planes[3]) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  const int sub_w = xstart < v->width ? (v->width - xstart + xadd - 1) / xadd : 0;
  const int sub_h = ystart < v->height ? (v->height - ystart + yadd - 1) / yadd : 0;
  if (v->blocks.empty()) return SFRT_E_EMPTY;
  if (sub_w == 0 || sub_h == 0) return SFRT_OK;
  if (!v->sample_grid_ok(sub_w, sub_h)) return SFRT_E_INVALID;
  sfrt::DeviceGuard g(v->device);
  const size_t px = (size_t)sub_w * sub_h;
  // the last update_image finished with the buffers (it waits for its copies)
  HIP_TRY(v->d_frame.reserve(px * 4, v->stream));
  for (int q = 0; planes && q < 4; q++)
    if (planes[q]) {
      HIP_TRY(v->d_aux[q].reserve(px * 4, v->stream));
      HIP_TRY(v->h_aux[q].reserve(px * 4));
    }
  sfrt::VoxAux aux{};
  if (planes) {  // compact planes beside the compact frame
    aux.depth = planes[0] ? v->d_aux[0].ptr<float>() : nullptr;
    aux.cell = planes[1] ? v->d_aux[1].ptr<int32_t>() : nullptr;
    aux.face = planes[2] ? v->d_aux[2].ptr<int32_t>() : nullptr;
    aux.steps = planes[3] ? v->d_aux[3].ptr<int32_t>() : nullptr;
    aux.depth_pitch = aux.cell_pitch = aux.face_pitch = aux.steps_pitch = sub_w;
  }
  sfrt::VoxFrame f;
  int rc = v->prepare(f, v->stream);
  if (rc) return rc;
  // Supersampled (S = 1 << ss): S x S samples per addressed pixel, start and strides in samples
  // (sfrt_device.h subset_index); d_frame, the copy and the scatter stay at output size.  A
  // subset of one column (row) never steps, so its stride, which may exceed the frame, is not
  // scaled up.
  const int ss = v->ss;
  f.xstart = xstart << ss; f.xadd = (ss && sub_w == 1 ? 1 : xadd) << ss;
  f.ystart = ystart << ss; f.yadd = (ss && sub_h == 1 ? 1 : yadd) << ss;
  f.sub_w = sub_w << ss;
  f.sub_row0 = 0;
  f.sub_rows = sub_h << ss;
  f.out = v->d_frame.ptr<uint32_t>();
  f.out_pitch = sub_w;
  if (sfrt::launch_voxel(f, v->stream, v->launch_event(), planes ? &aux : nullptr)) return SFRT_E_HIP;
  HIP_TRY(v->launched(v->stream));
  std::vector<uint32_t> stage(px);  // pageable colour staging (left as it is)
  HIP_TRY(hipMemcpyAsync(stage.data(), v->d_frame.ptr(), px * 4, hipMemcpyDeviceToHost, v->stream));
  for (int q = 0; planes && q < 4; q++)
    if (planes[q])
      HIP_TRY(hipMemcpyAsync(v->h_aux[q].ptr(), v->d_aux[q].ptr(), px * 4, hipMemcpyDeviceToHost,
                             v->stream));
  rc = v->read_status(v->stream);
  if (rc) return rc;  // SFRT_E_TEXEL included: neither pixels nor any plane is written
  const auto scatter = [&](const uint32_t* src, void* dst) {
    sfrt::scatter_subset(src, (uint8_t*)dst, (size_t)v->width, sub_w, sub_h, xstart, xadd, ystart, yadd);
  };
  scatter(stage.data(), pixels);
  for (int q = 0; planes && q < 4; q++)
    if (planes[q]) scatter(v->h_aux[q].ptr<uint32_t>(), planes[q]);
  return SFRT_OK;
}

int sfrt_voxel_update_image(sfrt_voxel* v, uint8_t* pixels, int ystart, int yadd, int xstart,
                            int xadd) {
  return update_image_body(v, pixels, nullptr, ystart, yadd, xstart, xadd);
}

int sfrt_voxel_update_image_aux(sfrt_voxel* v, uint8_t* pixels, float* depth, int32_t* cell,
                                int32_t* face, int32_t* steps, int ystart, int yadd, int xstart,
                                int xadd) {
  void* const planes[4] = {depth, cell, face, steps};
  return update_image_body(v, pixels, planes, ystart, yadd, xstart, xadd);
}

// sfrt_voxel_render_band and sfrt_voxel_render_band_aux (with_aux false for the plain call).
static int render_band_body(sfrt_voxel* v, void* dev_pixels, int64_t pitch_bytes,
                            const sfrt_voxel_aux_planes* aux, bool with_aux, int row0, int rows,
                            void* hip_stream) {
  if (!v || !dev_pixels || row0 < 0 || rows < 0 || pitch_bytes % 4 != 0) return SFRT_E_INVALID;
  if (with_aux && (!aux || (!aux->depth && !aux->cell && !aux->face && !aux->steps)))
    return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  if (pitch_bytes < (int64_t)v->width * 4 || row0 + rows > v->height) return SFRT_E_INVALID;
  sfrt::VoxAux a{};
  if (with_aux &&
      (!sfrt::aux_plane(aux->depth, aux->depth_pitch_bytes, v->width, a.depth, a.depth_pitch) ||
       !sfrt::aux_plane(aux->cell, aux->cell_pitch_bytes, v->width, a.cell, a.cell_pitch) ||
       !sfrt::aux_plane(aux->face, aux->face_pitch_bytes, v->width, a.face, a.face_pitch) ||
       !sfrt::aux_plane(aux->steps, aux->steps_pitch_bytes, v->width, a.steps, a.steps_pitch)))
    return SFRT_E_INVALID;
  if (rows == 0) return SFRT_OK;
  if (!v->sample_grid_ok(v->width, rows)) return SFRT_E_INVALID;
  sfrt::DeviceGuard g(v->device);
  hipStream_t s = (hipStream_t)hip_stream;
  sfrt::VoxFrame f;
  int rc = v->prepare(f, s);
  if (rc) return rc;
  // supersampled: the band's S * rows sample rows of the S * width sample frame (rays by the
  // global sample row: bands tile the frame); the buffer and its pitch in output pixels
  const int ss = v->ss;
  f.xstart = 0; f.xadd = 1 << ss; f.ystart = 0; f.yadd = 1 << ss;
  f.sub_w = v->width << ss;
  f.sub_row0 = row0 << ss;
  f.sub_rows = rows << ss;
  f.out = (uint32_t*)dev_pixels;
  f.out_pitch = pitch_bytes / 4;
  long long tiles = 0;
  // the same key with and without planes: an aux band and a plain band of one stream share a chain
  const long long key = v->tile_order_on ? sfrt::voxel_tile_key(f, &tiles) : 0;
  sfrt::TileSchedPtrs p;
  sfrt::TileSched& sched = v->scheds.chain[v->scheds.pick(s)];
  HIP_TRY(sched.begin(key, tiles, s, v->tile_order_on, p));
  p.link(f);
  const bool queued = sfrt::launch_voxel(f, s, v->launch_event(), with_aux ? &a : nullptr) == 0;
  HIP_TRY(sched.end(p, s, queued));
  if (!queued) return SFRT_E_HIP;
  HIP_TRY(v->launched(s));
  return SFRT_OK;
}

int sfrt_voxel_render_band(sfrt_voxel* v, void* dev_pixels, int64_t pitch_bytes, int row0, int rows,
                           void* hip_stream) {
  return render_band_body(v, dev_pixels, pitch_bytes, nullptr, false, row0, rows, hip_stream);
}

int sfrt_voxel_render_band_aux(sfrt_voxel* v, void* dev_pixels, int64_t pitch_bytes,
                               const sfrt_voxel_aux_planes* aux, int row0, int rows, void* hip_stream) {
  return render_band_body(v, dev_pixels, pitch_bytes, aux, true, row0, rows, hip_stream);
}

// sfrt_voxel_render_subset and sfrt_voxel_render_subset_aux (with_aux false for the plain call):
// update_image's subset walk, stored in place in the caller's whole device frame (the placing
// kernels, voxel_trace.h launch_voxel) on the caller's stream; row-major, no tile-order chain.
static int render_subset_body(sfrt_voxel* v, void* dev_frame, int64_t pitch_bytes,
                              const sfrt_voxel_aux_planes* aux, bool with_aux, int ystart, int yadd,
                              int xstart, int xadd, void* hip_stream) {
  if (!v || !dev_frame || ystart < 0 || xstart < 0 || yadd <= 0 || xadd <= 0 || pitch_bytes % 4 != 0)
    return SFRT_E_INVALID;
  if (with_aux && (!aux || (!aux->depth && !aux->cell && !aux->face && !aux->steps)))
    return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  // the world's own validation first, then the sizes that need the world's width: the order of
  // sfrt_world_render_subset
  if (v->blocks.empty()) return SFRT_E_EMPTY;
  if (pitch_bytes < (int64_t)v->width * 4) return SFRT_E_INVALID;
  sfrt::VoxAux a{};
  if (with_aux &&
      (!sfrt::aux_plane(aux->depth, aux->depth_pitch_bytes, v->width, a.depth, a.depth_pitch) ||
       !sfrt::aux_plane(aux->cell, aux->cell_pitch_bytes, v->width, a.cell, a.cell_pitch) ||
       !sfrt::aux_plane(aux->face, aux->face_pitch_bytes, v->width, a.face, a.face_pitch) ||
       !sfrt::aux_plane(aux->steps, aux->steps_pitch_bytes, v->width, a.steps, a.steps_pitch)))
    return SFRT_E_INVALID;
  // 64-bit: a stride near INT_MAX is a valid one-pixel subset
  const int sub_w = xstart < v->width ? (int)(((long long)v->width - xstart + xadd - 1) / xadd) : 0;
  const int sub_h = ystart < v->height ? (int)(((long long)v->height - ystart + yadd - 1) / yadd) : 0;
  if (sub_w == 0 || sub_h == 0) return SFRT_OK;
  if (!v->sample_grid_ok(sub_w, sub_h)) return SFRT_E_INVALID;
  sfrt::DeviceGuard g(v->device);
  hipStream_t s = (hipStream_t)hip_stream;
  sfrt::VoxFrame f;
  int rc = v->prepare(f, s);
  if (rc) return rc;
  // the subset as update_image_body takes it (supersampled: in samples, a stride that addresses
  // one pixel only not scaled)
  const int ss = v->ss;
  f.xstart = xstart << ss; f.xadd = (ss && sub_w == 1 ? 1 : xadd) << ss;
  f.ystart = ystart << ss; f.yadd = (ss && sub_h == 1 ? 1 : yadd) << ss;
  f.sub_w = sub_w << ss;
  f.sub_row0 = 0;
  f.sub_rows = sub_h << ss;
  // Pixel (xstart + k xadd, ystart + l yadd) of the frame is output pixel (k, l) of the subset:
  // base frame + ystart * pitch + xstart, row stride yadd * pitch, column stride xadd (elements).
  // A subset of one column (row) never applies its stride, which is then passed as 1.
  const long long pitch = pitch_bytes / 4;
  const int col_stride = sub_w == 1 ? 1 : xadd;
  const long long row_mul = sub_h == 1 ? 1 : yadd;
  f.out = (uint32_t*)dev_frame + (long long)ystart * pitch + xstart;
  f.out_pitch = row_mul * pitch;
  if (with_aux) {
    if (a.depth) a.depth += (long long)ystart * a.depth_pitch + xstart;
    if (a.cell) a.cell += (long long)ystart * a.cell_pitch + xstart;
    if (a.face) a.face += (long long)ystart * a.face_pitch + xstart;
    if (a.steps) a.steps += (long long)ystart * a.steps_pitch + xstart;
    a.depth_pitch *= row_mul; a.cell_pitch *= row_mul; a.face_pitch *= row_mul; a.steps_pitch *= row_mul;
  }
  if (sfrt::launch_voxel(f, s, v->launch_event(), with_aux ? &a : nullptr, col_stride)) return SFRT_E_HIP;
  HIP_TRY(v->launched(s));
  return SFRT_OK;
}

int sfrt_voxel_render_subset(sfrt_voxel* v, void* dev_frame, int64_t pitch_bytes, int ystart, int yadd,
                             int xstart, int xadd, void* hip_stream) {
  return render_subset_body(v, dev_frame, pitch_bytes, nullptr, false, ystart, yadd, xstart, xadd,
                            hip_stream);
}

int sfrt_voxel_render_subset_aux(sfrt_voxel* v, void* dev_frame, int64_t pitch_bytes,
                                 const sfrt_voxel_aux_planes* aux, int ystart, int yadd, int xstart,
                                 int xadd, void* hip_stream) {
  return render_subset_body(v, dev_frame, pitch_bytes, aux, true, ystart, yadd, xstart, xadd,
                            hip_stream);
}

// sfrt_voxel_render_views and sfrt_voxel_render_views_aux (with_aux false for the plain call): view
// k is the whole frame that set_camera(views[k].cam) [+ set_dynamics(sort_dynamics(the world's
// list, the view's camera)) with DYNAMICS] + render_band[_aux] would write, all views in one launch
// of the view kernels (voxel_trace.h launch_voxel_views).  The per-camera state of a band -- the
// col and row tables, the billboards with atan_b (in the view's own order and with its own
// distToCamera under DYNAMICS), dda_qlim -- is built per view by the functions prepare() builds
// the band's with, into one pinned block:
//   count view records | col tables | row tables | count dyn tables | the lights, once
// (16-byte aligned parts; views with the same rotation and fov_h share a col table, with the same
// hrotation and fov_v a row table: the bytes are a function of those and the size alone), sent by
// one copy on the caller's stream from a slot of the view ring.  Nothing of the world is written:
// not the camera, the list or its order, nor the band's staged tables (cur_slot, staged_version) --
// but a pending set_blocks rewrite is carried out, as by a band.
static int render_views_body(sfrt_voxel* v, const sfrt_view* views,
                             const sfrt_voxel_aux_planes* planes, bool with_aux, int count,
                             int64_t pitch_bytes, int flags, void* hip_stream) {
  if (!v || !views || count < 0 || count > SFRT_MAX_VIEWS ||
      (flags & ~SFRT_VOXEL_VIEWS_DYNAMICS) != 0 || pitch_bytes % 4 != 0 || (with_aux && !planes))
    return SFRT_E_INVALID;
  for (int k = 0; k < count; k++) {
    if (!views[k].dev_pixels || !sfrt::aligned4({views[k].dev_pixels}) || !camera_ok(views[k].cam))
      return SFRT_E_INVALID;
    if (with_aux && !planes[k].depth && !planes[k].cell && !planes[k].face && !planes[k].steps)
      return SFRT_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(v->mu);
  if (count == 0) return SFRT_OK;
  if (v->width <= 0 || v->height <= 0 || pitch_bytes < (int64_t)v->width * 4) return SFRT_E_INVALID;
  std::vector<sfrt::VoxAux> aux(with_aux ? (size_t)count : 0);
  for (size_t k = 0; k < aux.size(); k++) {
    const sfrt_voxel_aux_planes& p = planes[k];
    sfrt::VoxAux& a = aux[k];
    if (!sfrt::aux_plane(p.depth, p.depth_pitch_bytes, v->width, a.depth, a.depth_pitch) ||
        !sfrt::aux_plane(p.cell, p.cell_pitch_bytes, v->width, a.cell, a.cell_pitch) ||
        !sfrt::aux_plane(p.face, p.face_pitch_bytes, v->width, a.face, a.face_pitch) ||
        !sfrt::aux_plane(p.steps, p.steps_pitch_bytes, v->width, a.steps, a.steps_pitch))
      return SFRT_E_INVALID;
  }
  if (!v->sample_grid_ok(v->width, v->height)) return SFRT_E_INVALID;
  // The frame geometry of render_band_body for rows [0, height), the same for every view, and the
  // grid it gives, refused before anything is queued if one launch cannot take it.
  const int ss = v->ss;
  const int W = v->width << ss, H = v->height << ss;
  sfrt::VoxFrame f;
  v->begin_frame(f);
  f.xstart = 0; f.xadd = 1 << ss; f.ystart = 0; f.yadd = 1 << ss;
  f.sub_w = W;
  f.sub_row0 = 0;
  f.sub_rows = H;
  f.out_pitch = pitch_bytes / 4;
  if (!sfrt::voxel_views_grid_ok(f, count)) return SFRT_E_INVALID;
  if (v->blocks.empty()) return SFRT_E_EMPTY;
  sfrt::DeviceGuard g(v->device);
  hipStream_t s = (hipStream_t)hip_stream;  // HIP convention: NULL = the null stream
  const bool sorted = (flags & SFRT_VOXEL_VIEWS_DYNAMICS) != 0;
  // which earlier view's col (row) table a view shares: the first with the same inputs, bit for bit
  const auto same = [](float a, float b) { return std::memcmp(&a, &b, 4) == 0; };
  std::vector<int> col_of((size_t)count), row_of((size_t)count);
  int ncol = 0, nrow = 0;
  for (int k = 0; k < count; k++) {
    const sfrt_camera& c = views[k].cam;
    col_of[k] = row_of[k] = -1;
    for (int j = 0; j < k && (col_of[k] < 0 || row_of[k] < 0); j++) {
      const sfrt_camera& o = views[j].cam;
      if (col_of[k] < 0 && same(c.rotation, o.rotation) && same(c.fov_h, o.fov_h)) col_of[k] = col_of[j];
      if (row_of[k] < 0 && same(c.hrotation, o.hrotation) && same(c.fov_v, o.fov_v)) row_of[k] = row_of[j];
    }
    if (col_of[k] < 0) col_of[k] = ncol++;
    if (row_of[k] < 0) row_of[k] = nrow++;
  }
  const size_t nd = v->dyn.size(), nl = v->lights.size();
  const size_t b_rec = up16((size_t)count * sizeof(sfrt::VoxViewRec));
  const size_t b_col = up16((size_t)W * 3 * sizeof(float)), b_row = up16((size_t)H * 2 * sizeof(float)),
               b_dyn = up16(nd * sizeof(sfrt::VoxDyn)), b_lit = up16(nl * sizeof(sfrt::VoxLight));
  const size_t at_col = b_rec, at_row = at_col + (size_t)ncol * b_col,
               at_dyn = at_row + (size_t)nrow * b_row, at_lit = at_dyn + (size_t)count * b_dyn;
  const size_t bytes = at_lit + b_lit + 16;
  sfrt::TableSlot& t = v->slots[sfrt_voxel::kSlots + v->next_view_slot];
  v->next_view_slot = (v->next_view_slot + 1) % sfrt_voxel::kViewSlots;
  HIP_TRY(t.reclaim());  // the launch that read the slot's last block is done (no device-wide wait)
  HIP_TRY(t.grow(bytes, s));
  uint8_t* const h = t.h.ptr<uint8_t>();
  uint8_t* const d = t.d.ptr<uint8_t>();
  std::vector<float> col_xmax((size_t)ncol, -1.0f), row_xmax((size_t)nrow, -1.0f);  // -1: not built
  std::vector<sfrt_dynamic> list;
  for (int k = 0; k < count; k++) {
    const sfrt_camera& cam = views[k].cam;
    const size_t c_at = at_col + (size_t)col_of[k] * b_col, r_at = at_row + (size_t)row_of[k] * b_row,
                 d_at = at_dyn + (size_t)k * b_dyn;
    if (col_xmax[col_of[k]] < 0.0f) col_xmax[col_of[k]] = col_table(cam, W, (float*)(h + c_at));
    if (row_xmax[row_of[k]] < 0.0f) row_xmax[row_of[k]] = row_table(cam, H, (float*)(h + r_at));
    const sfrt_dynamic* dyn = v->dyn.data();
    if (sorted) {  // from the world's list every time, not from view k-1's
      list = v->dyn;
      sort_dynamics(list.data(), nd, cam.pos);
      dyn = list.data();
    }
    dyn_table(cam, dyn, nd, (sfrt::VoxDyn*)(h + d_at));
    sfrt::VoxViewRec r;
    std::memset(&r, 0, sizeof r);
    r.cam[0] = cam.pos[0]; r.cam[1] = cam.pos[1]; r.cam[2] = cam.pos[2];
    r.dda_qlim = dda_qlim(r.cam, f.maxiter, std::max(col_xmax[col_of[k]], row_xmax[row_of[k]]));
    r.col = (const float*)(d + c_at);
    r.row = (const float*)(d + r_at);
    r.dyn = (const sfrt::VoxDyn*)(d + d_at);
    r.out = (uint32_t*)views[k].dev_pixels;
    if (with_aux) r.aux = aux[(size_t)k];
    std::memcpy(h + (size_t)k * sizeof r, &r, sizeof r);
  }
  light_table(v->lights.data(), nl, (sfrt::VoxLight*)(h + at_lit));
  HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  // the copy is queued: on any failure below the slot stays busy until it has run
  int rc = v->blocks_upload(s);  // before fill_world: it reads d_cells
  if (rc == SFRT_OK && v->shared.before_read(s) != hipSuccess) rc = SFRT_E_HIP;
  if (rc == SFRT_OK) {
    v->fill_world(f);
    f.lights = (const sfrt::VoxLight*)(d + at_lit);
    if (sfrt::launch_voxel_views(f, (const sfrt::VoxViewRec*)d, count, with_aux, s, t.launch_event()))
      rc = SFRT_E_HIP;
  }
  if (rc != SFRT_OK) {
    (void)t.staged(s);
    return rc;
  }
  HIP_TRY(t.launched_with(s));
  return SFRT_OK;
}

int sfrt_voxel_render_views(sfrt_voxel* v, const sfrt_view* views, int count, int64_t pitch_bytes,
                            int flags, void* hip_stream) {
  return render_views_body(v, views, nullptr, false, count, pitch_bytes, flags, hip_stream);
}

int sfrt_voxel_render_views_aux(sfrt_voxel* v, const sfrt_view* views,
                                const sfrt_voxel_aux_planes* planes, int count, int64_t pitch_bytes,
                                int flags, void* hip_stream) {
  return render_views_body(v, views, planes, true, count, pitch_bytes, flags, hip_stream);
}

int sfrt_voxel_sort_dynamics(sfrt_dynamic* dyn, int count, const float cam_pos[3]) {
  if (count < 0 || (count > 0 && (!dyn || !cam_pos))) return SFRT_E_INVALID;
  sort_dynamics(dyn, (size_t)count, cam_pos);
  return SFRT_OK;
}

// ---- batched ray queries (include/sfrt.h) ----
namespace {

static_assert(SFRT_VOXEL_MAX_SHADOW_DIST == sfrt::kVoxMaxShadowDist, "one bound, two headers");

// The argument checks the host and the device call share; the world's own come with its mutex held.
int cast_rays_args(const sfrt_voxel* v, const float* dirs, const float* yscales, const float* origins,
                   int64_t count, const sfrt_voxel_ray_hits* out) {
  if (!v || !dirs || !out || count < 0 || count > 0x7fffffffLL) return SFRT_E_INVALID;
  if (!out->pos && !out->depth && !out->cell && !out->face && !out->steps && !out->rgba)
    return SFRT_E_INVALID;
  if (!sfrt::aligned4({dirs, yscales, origins, out->pos, out->depth, out->cell, out->face, out->steps, out->rgba}))
    return SFRT_E_INVALID;
  return SFRT_OK;
}
int shadow_rays_args(const sfrt_voxel* v, const float* origins, const float* dirs,
                     const float* max_dists, int64_t count, const int32_t* free_, const int32_t* steps) {
  if (!v || !origins || !dirs || !max_dists || count < 0 || count > 0x7fffffffLL) return SFRT_E_INVALID;
  if (!free_ && !steps) return SFRT_E_INVALID;
  if (!sfrt::aligned4({origins, dirs, max_dists, free_, steps})) return SFRT_E_INVALID;
  return SFRT_OK;
}
// What a batch needs of the world (mutex held), before anything is queued.
int rays_world(const sfrt_voxel* v) {
  if (v->blocks.empty()) return SFRT_E_EMPTY;
  // prepare() stages the frame tables too (a batch counts as a frame call): their size must fit
  if (v->width <= 0 || v->height <= 0 || !v->sample_grid_ok(1, 1)) return SFRT_E_INVALID;
  return SFRT_OK;
}

// One launch of the ray-batch kernel on s with the world's mutex held: the frame fill's snapshot
// (prepare: the deferred grid upload, the staged tables, camera and view distances) and nothing
// of the tile-order chains.
int cast_rays_launch(sfrt_voxel* v, const float* dev_dirs, const float* dev_yscales,
                     const float* dev_origins, int64_t count, const sfrt_voxel_ray_hits& out,
                     hipStream_t s) {
  sfrt::VoxFrame f;
  const int rc = v->prepare(f, s);
  if (rc) return rc;
  sfrt::VoxRays a{};
  a.dirs = dev_dirs;
  a.yscales = dev_yscales;
  a.origins = dev_origins;
  a.count = count;
  a.pos = out.pos;
  a.depth = out.depth;
  a.cell = out.cell;
  a.face = out.face;
  a.steps = out.steps;
  a.rgba = (uint32_t*)out.rgba;
  if (sfrt::launch_voxel_rays(f, a, s, v->launch_event())) return SFRT_E_HIP;
  HIP_TRY(v->launched(s));
  return SFRT_OK;
}
int shadow_rays_launch(sfrt_voxel* v, const float* dev_origins, const float* dev_dirs,
                       const float* dev_max_dists, int64_t count, int32_t* dev_free,
                       int32_t* dev_steps, hipStream_t s) {
  sfrt::VoxFrame f;
  const int rc = v->prepare(f, s);
  if (rc) return rc;
  sfrt::VoxShadowRays a{};
  a.origins = dev_origins;
  a.dirs = dev_dirs;
  a.max_dists = dev_max_dists;
  a.count = count;
  a.free_ = dev_free;
  a.steps = dev_steps;
  if (sfrt::launch_voxel_shadow_rays(f, a, s, v->launch_event())) return SFRT_E_HIP;
  HIP_TRY(v->launched(s));
  return SFRT_OK;
}

}  // namespace

int sfrt_voxel_cast_rays_device(sfrt_voxel* v, const float* dev_dirs, const float* dev_yscales,
                                const float* dev_origins, int64_t count,
                                const sfrt_voxel_ray_hits* dev_out, void* hip_stream) {
  int rc = cast_rays_args(v, dev_dirs, dev_yscales, dev_origins, count, dev_out);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(v->mu);
  if (count == 0) return SFRT_OK;
  if ((rc = rays_world(v))) return rc;
  sfrt::DeviceGuard g(v->device);
  return cast_rays_launch(v, dev_dirs, dev_yscales, dev_origins, count, *dev_out, (hipStream_t)hip_stream);
}

int sfrt_voxel_cast_rays(sfrt_voxel* v, const float* dirs, const float* yscales, const float* origins,
                         int64_t count, const sfrt_voxel_ray_hits* out) {
  int rc = cast_rays_args(v, dirs, yscales, origins, count, out);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(v->mu);
  if (count == 0) return SFRT_OK;
  if ((rc = rays_world(v))) return rc;
  sfrt::DeviceGuard g(v->device);
  const sfrt::BatchLayout l((size_t)count, {{dirs, 12}, {yscales, 4}, {origins, 12}},
                            {{out->pos, 12}, {out->depth, 4}, {out->cell, 4}, {out->face, 4},
                             {out->steps, 4}, {out->rgba, 4}});
  HIP_TRY(v->ray_stage.upload(l, v->stream));
  void* const d = v->ray_stage.d.ptr();
  const sfrt_voxel_ray_hits dev{l.out_at<float>(d, 0), l.out_at<float>(d, 1), l.out_at<int32_t>(d, 2),
                                l.out_at<int32_t>(d, 3), l.out_at<int32_t>(d, 4), l.out_at<uint8_t>(d, 5)};
  if ((rc = cast_rays_launch(v, l.in_at<float>(d, 0), l.in_at<float>(d, 1), l.in_at<float>(d, 2),
                             count, dev, v->stream)))
    return rc;
  HIP_TRY(v->ray_stage.download(l, v->stream));
  rc = v->read_status(v->stream);
  if (rc) return rc;  // SFRT_E_TEXEL included: no output is written, as sfrt_voxel_update_image_aux
  l.copy_outputs(v->ray_stage.h.ptr());
  return SFRT_OK;
}

int sfrt_voxel_cast_shadow_rays_device(sfrt_voxel* v, const float* dev_origins, const float* dev_dirs,
                                       const float* dev_max_dists, int64_t count, int32_t* dev_free,
                                       int32_t* dev_steps, void* hip_stream) {
  int rc = shadow_rays_args(v, dev_origins, dev_dirs, dev_max_dists, count, dev_free, dev_steps);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(v->mu);
  if (count == 0) return SFRT_OK;
  if ((rc = rays_world(v))) return rc;
  sfrt::DeviceGuard g(v->device);
  return shadow_rays_launch(v, dev_origins, dev_dirs, dev_max_dists, count, dev_free, dev_steps,
                            (hipStream_t)hip_stream);
}

int sfrt_voxel_cast_shadow_rays(sfrt_voxel* v, const float* origins, const float* dirs,
                                const float* max_dists, int64_t count, int32_t* free_, int32_t* steps) {
  int rc = shadow_rays_args(v, origins, dirs, max_dists, count, free_, steps);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(v->mu);
  if (count == 0) return SFRT_OK;
  if ((rc = rays_world(v))) return rc;
  sfrt::DeviceGuard g(v->device);
  const sfrt::BatchLayout l((size_t)count, {{origins, 12}, {dirs, 12}, {max_dists, 4}},
                            {{free_, 4}, {steps, 4}});
  HIP_TRY(v->ray_stage.upload(l, v->stream));
  void* const d = v->ray_stage.d.ptr();
  if ((rc = shadow_rays_launch(v, l.in_at<float>(d, 0), l.in_at<float>(d, 1), l.in_at<float>(d, 2),
                               count, l.out_at<int32_t>(d, 0), l.out_at<int32_t>(d, 1), v->stream)))
    return rc;
  HIP_TRY(v->ray_stage.download(l, v->stream));
  HIP_TRY(hipStreamSynchronize(v->stream));  // no status: a shadow ray reads no texel
  l.copy_outputs(v->ray_stage.h.ptr());
  return SFRT_OK;
}

int sfrt_voxel_set_option(sfrt_voxel* v, int option, int value) {
  if (!v) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  if (option == SFRT_OPT_TILE_ORDER) {
    v->tile_order_on = value == 2 ? 2 : value ? 1 : 0;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_SUPERSAMPLE) {
    if (value != 1 && value != 2 && value != 4) return SFRT_E_INVALID;
    const int ss = value == 4 ? 2 : value == 2 ? 1 : 0;
    if (ss != v->ss) v->tables_version++;  // the col / row tables (and dda_qlim's xmax) are per sample
    v->ss = ss;
    return SFRT_OK;
  }
  return SFRT_E_INVALID;
}

int sfrt_voxel_get_option(const sfrt_voxel* v, int option, int* value) {
  if (!v || !value) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  switch (option) {
    case SFRT_OPT_TILE_ORDER: *value = v->tile_order_on; return SFRT_OK;
    case SFRT_OPT_SUPERSAMPLE: *value = 1 << v->ss; return SFRT_OK;
    default: return SFRT_E_INVALID;
  }
}

int sfrt_voxel_check(sfrt_voxel* v, void* hip_stream) {
  if (!v) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(v->mu);
  sfrt::DeviceGuard g(v->device);
  return v->read_status((hipStream_t)hip_stream);
}

}  // extern "C"
