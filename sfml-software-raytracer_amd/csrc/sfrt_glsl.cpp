// sfrt_glsl.cpp -- host side of the GLSL renderer: the
// shader's uniform state, the `ground` texture with its mip chain, and the
// extern "C" entry points sfrt_glsl_* of include/sfrt.h.
//
// Reference (paths under /root/reference/Raytracing/):
//   uniforms                        rayShader.frag:1-11
//   upload by name                  SphereWorld.cpp:214-238 (UpdateSpheres), Source.cpp:143-146
//   ground: Floor.png, REPEAT, mips SphereWorld.cpp:52-57
//   rt.draw(sp, &world.shader)      Source.cpp:150-153 (one fragment per render-target pixel)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "glsl_trace.h"
#include "sfrt.h"
#include "sfrt_host.h"
#include "sfrt_sched.h"
#include "sfrt_math.h"

#pragma clang fp contract(off)

namespace {

// Uniform values are bounded so that every product in the wall pass stays
// finite (the kernel's step-0 shortcut relies on it).
constexpr float kUniformBound = 1e15f;

bool bounded(float v) { return std::fabs(v) <= kUniformBound; }  // false for NaN

// Largest binary32 s >= 0 with sqrtf(s) <= r (-1 when there is none):
// step(length(rpos), r) == 1  <=>  dot(rpos, rpos) <= s_in (sqrtf is monotone).
float inside_bound(float r) {
  if (!(std::sqrt(0.0f) <= r)) return -1.0f;
  uint32_t lo = 0, hi = 0x7f7fffffu;  // sqrt(lo) <= r holds; find the last such bit pattern
  auto ok = [r](uint32_t b) { return std::sqrt(sfrt_math::u2f(b)) <= r; };
  if (ok(hi)) return sfrt_math::u2f(hi);
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ok(mid)) lo = mid; else hi = mid;
  }
  return sfrt_math::u2f(lo);
}

// generateMipmap() as DESIGN.md 4b fixes it: 2x2 (2x1, 1x2) box average,
// rounded half up, down to 1x1.  Power-of-two sides.
void build_mips(const uint8_t* rgba, int w, int h, std::vector<uint32_t>& out, int* lw, int* lh,
                int* off, int* levels) {
  std::vector<uint8_t> cur(rgba, rgba + (size_t)w * h * 4);
  out.clear();
  int k = 0;
  for (;;) {
    lw[k] = w;
    lh[k] = h;
    off[k] = (int)out.size();
    for (size_t p = 0; p < (size_t)w * h; p++) {
      uint32_t v;
      std::memcpy(&v, &cur[p * 4], 4);
      out.push_back(v);
    }
    if (w == 1 && h == 1) break;
    const int nw = w > 1 ? w / 2 : 1, nh = h > 1 ? h / 2 : 1;
    const int fx = w > 1 ? 2 : 1, fy = h > 1 ? 2 : 1, n = fx * fy;
    std::vector<uint8_t> nxt((size_t)nw * nh * 4);
    for (int y = 0; y < nh; y++)
      for (int x = 0; x < nw; x++)
        for (int c = 0; c < 4; c++) {
          int sum = 0;
          for (int dy = 0; dy < fy; dy++)
            for (int dx = 0; dx < fx; dx++)
              sum += cur[((size_t)(y * fy + dy) * w + (x * fx + dx)) * 4 + c];
          nxt[((size_t)y * nw + x) * 4 + c] = (uint8_t)((sum + n / 2) / n);
        }
    cur.swap(nxt);
    w = nw;
    h = nh;
    k++;
  }
  *levels = k + 1;
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

struct sfrt_glsl {
  int device = 0;
  sfrt_glsl_uniforms u{};
  int ground_w = 0, ground_h = 0;
  // SFRT_OPT_TILE_ORDER (sfrt_glsl_draw): on by default since round 4 (1080p -6 %, 4K -1 %, also
  // with the world moving every frame: profiles/ab/r4_ab9); draw_image stays row-major
  int tile_order_on = 1;
  // SFRT_OPT_SUPERSAMPLE: log2 of the factor S (0, 1, 2).  S > 1: a draw renders the S * width x
  // S * height target with `size` scaled by S (exact in binary32) and box-filters it in the kernel
  int ss = 0;
  // adaptive tile order (sfrt_sched.h), one chain per stream: draws on two streams share no order
  // or cost buffer, so neither waits on the host for the other (as the sphere world, since round 6)
  sfrt::TileChains scheds;
  // device resources
  hipStream_t stream = nullptr;
  uint32_t* d_mip = nullptr;
  // set_ground is stream-ordered: the new chain goes up on `stream` behind every draw that read
  // the old one (through the table slots' events), and draws on other streams wait for it
  sfrt::SharedBuffer ground;
  sfrt::PinnedStage mip_stage;
  int mip_levels = 0;
  int mip_w[sfrt::kGlslMipLevels] = {}, mip_h[sfrt::kGlslMipLevels] = {},
      mip_off[sfrt::kGlslMipLevels] = {};
  // Per-draw tables (walls | balls | pairs | mats) in a ring of slots, each
  // with a pinned staging copy and the event of the last draw that read it,
  // so draws on different streams never overwrite tables still in use.
  // (sfrt::TableSlot, sfrt_host.h: a reuse on another stream waits for the slot's last user.)
  // The view batches (sfrt_glsl_render_views) stage their block -- view records and a table block
  // of their own -- in a ring of their own behind the draws' slots, in the same array so that
  // set_ground waits for the batches that read the old chain too; a batch never touches the
  // draws' slots, cur_slot or staged_version.
  static constexpr int kSlots = 4, kViewSlots = 4;
  sfrt::TableSlot slots[kSlots + kViewSlots];
  int next_slot = 0;
  int cur_slot = -1;
  int next_view_slot = 0;
  // The tables depend only on the uniform block: every uniform setter bumps u_version, and a
  // draw with the uniforms unchanged since the last staging reuses that slot (no host table
  // build, no copy in front of the kernel).
  uint64_t u_version = 1, staged_version = 0;
  size_t staged_off[3] = {0, 0, 0};  // byte offsets of balls | pairs | mats in the staged slot
  int* d_status = nullptr;
  // draw_image's device frame and, per requested plane of sfrt_glsl_draw_image_aux (depth, sphere,
  // steps), a compact device plane; the staging of sfrt_glsl_cast_rays (the host call): a batch's
  // directions and its requested outputs.  All on `stream` (sfrt_host.h DeviceBuf); the host side
  // of each copy is the caller's pageable memory (left as it is).
  sfrt::DeviceBuf d_frame, d_aux[3], d_rays;
  sfrt::Relay relay;         // events recorded on callers' streams, relayed (sfrt_host.h)
  mutable std::mutex mu;

  sfrt_glsl() {
    for (auto& t : slots) t.relay = &relay;
    ground.relay = &relay;
  }

  ~sfrt_glsl() {
    sfrt::DeviceGuard g(device);
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipDeviceSynchronize();
    scheds.release();
    (void)hipFree(d_mip);
    mip_stage.release();
    ground.release();
    for (auto& t : slots) t.release();
    relay.release();
    (void)hipFree(d_status);
    d_frame.release();
    for (sfrt::DeviceBuf& p : d_aux) p.release();
    d_rays.release();
    if (stream) (void)hipStreamDestroy(stream);
  }

  // What validate() asks of the three camera uniforms, for values that are not (yet) uniforms:
  // the views of a batch.
  static bool camera_ok(const float* campos, const float* rotation, const float* fov) {
    for (float c : {campos[0], campos[1], campos[2], rotation[0], rotation[1], fov[0], fov[1]})
      if (!bounded(c)) return false;
    return true;
  }

  // view: the uniforms only a frame reads (rotation, fov, size); a ray batch reads none of them.
  // camera false: a view batch, which brings campos, rotation and fov of its own (camera_ok).
  int validate(bool view = true, bool camera = true) const {
    const sfrt_glsl_uniforms& v = u;
    if (v.sphere_count < 0 || v.light_count < 0 || v.all_spheres_count > SFRT_GLSL_MAX_SPHERES ||
        v.sphere_count + v.light_count > v.all_spheres_count)
      return SFRT_E_INVALID;
    if (camera)
      for (float c : {v.campos[0], v.campos[1], v.campos[2]})
        if (!bounded(c)) return SFRT_E_INVALID;
    if (view) {
      if (camera)
        for (float c : {v.rotation[0], v.rotation[1], v.fov[0], v.fov[1]})
          if (!bounded(c)) return SFRT_E_INVALID;
      if (!(v.size[0] > 0.0f && v.size[1] > 0.0f && bounded(v.size[0]) && bounded(v.size[1])))
        return SFRT_E_INVALID;
      // the `size` the supersampled fragments see
      if (!bounded(v.size[0] * (float)(1 << ss)) || !bounded(v.size[1] * (float)(1 << ss)))
        return SFRT_E_INVALID;
    }
    for (int k = 0; k < v.all_spheres_count; k++)
      for (int c = 0; c < 4; c++)
        if (!bounded(v.spheres[k][c]) || !bounded(v.uvs[k][c]) || !bounded(v.lights[k][c]))
          return SFRT_E_INVALID;
    return SFRT_OK;
  }

  // The wall records of the uniform block (at least one entry, for an empty table's sake).
  std::vector<sfrt::GlslWall> wall_table() const {
    const int sc = u.sphere_count;
    std::vector<sfrt::GlslWall> walls(sc > 0 ? sc : 1);
    for (int k = 0; k < sc; k++) {
      const float* S = u.spheres[k];
      walls[k] = {S[0], S[1], S[2], S[3], S[3] * S[3], inside_bound(S[3]), 0.0f, 0.0f};
    }
    return walls;
  }

  // The per-camera part of a frame record, from what the three camera uniforms hold (a draw: the
  // shader's own; a view batch: each view's, once per view) and the `size` uniform: the basis,
  // fov_x / fov_y / hk / vk, campos, cam_negzero, wall_start and wall_cull_margin.  CAM is the
  // frame record itself or a view's record (sfrt::GlslViewRec: the same field names).  frame false:
  // a ray batch, which reads neither hk nor vk.
  template <class CAM>
  void camera_terms(const float* campos, const float* rotation, const float* fov, bool frame,
                    const std::vector<sfrt::GlslWall>& walls, CAM& f) const {
    const sfrt_glsl_uniforms& v = u;
    const int sc = v.sphere_count;
    // main(), rayShader.frag:165-173 -- VRotateX / VRotateY (:16-25) on unit axes
    auto rot_x = [](const float* a, float amount, float* o) {
      const float s = std::sin(amount), c = std::cos(amount);
      o[0] = a[0];
      o[1] = a[1] * c - a[2] * s;
      o[2] = a[1] * s + a[2] * c;
    };
    auto rot_y = [](const float* a, float amount, float* o) {
      const float s = std::sin(amount), c = std::cos(amount);
      o[0] = a[0] * c + a[2] * s;
      o[1] = a[1];
      o[2] = -a[0] * s + a[2] * c;
    };
    const float ey[3] = {0, 1, 0}, ez[3] = {0, 0, 1}, ex[3] = {1, 0, 0};
    float up0[3], fwd0[3];
    rot_x(ey, -rotation[1], up0);
    rot_x(ez, -rotation[1], fwd0);
    rot_y(ex, rotation[0], f.right);
    rot_y(fwd0, rotation[0], f.fwd);
    rot_y(up0, rotation[0], f.up);
    for (int c = 0; c < 3; c++) f.campos[c] = campos[c];
    f.fov_x = fov[0];
    f.fov_y = fov[1];
    // size of the S * width x S * height target when supersampled (a power of two: exact)
    if (frame) {
      f.hk = fov[0] / (v.size[0] * (float)(1 << ss)) * 2.0f;
      f.vk = fov[1] / (v.size[1] * (float)(1 << ss)) * 2.0f;
    }
    f.cam_negzero = (std::signbit(campos[0]) && campos[0] == 0.0f) ||
                    (std::signbit(campos[1]) && campos[1] == 0.0f) ||
                    (std::signbit(campos[2]) && campos[2] == 0.0f);
    // Every lane starts at campos: the wall-pass iterations before the first
    // wall containing campos (same test as the kernel) are no-ops for all of
    // them.  With a -0.0 in campos the kernel's literal update runs from 0.
    f.wall_start = 0;
    if (!f.cam_negzero && sc > 0) {
      int j = 0;
      for (; j < sc; j++) {
        const float rx = campos[0] - walls[j].x, ry = campos[1] - walls[j].y,
                    rz = campos[2] - walls[j].z;
        if ((rx * rx + ry * ry) + rz * rz <= walls[j].s_in) break;
      }
      f.wall_start = j < sc ? j : 3 * sc;  // inside no wall: no lane ever moves
    }
    // The wall cull's margin: every wall-pass position lies inside (or on) some wall reached from
    // campos, so its coordinates are bounded by R = max(|campos|, max_k |c_k| + r_k); the
    // positions' binary32 drift over <= 3 sc moves (an add and a multiply each, each rounding
    // within 2^-24 R) stays below 2 * 3 * sc * 2^-24 R < 2.3e-5 R for sc <= 64
    static_assert(2.0 * 3.0 * 64.0 * 0x1.0p-24 < 1e-3 / 8, "the margin dwarfs the drift");
    f.wall_cull_margin = 0.0f;
    if (!f.cam_negzero && sc > 0 && sc <= 64) {
      double R = std::max({std::fabs((double)campos[0]), std::fabs((double)campos[1]),
                           std::fabs((double)campos[2])});
      for (int k = 0; k < sc; k++)
        for (int c = 0; c < 3; c++)
          R = std::max(R, std::fabs((double)v.spheres[k][c]) + std::fabs((double)v.spheres[k][3]));
      const double m = 1e-3 * R + 1e-4;
      if (std::isfinite(m) && m < 1e30) f.wall_cull_margin = (float)m;
    }
  }

  // Byte offsets of balls | pairs | mats behind the walls in a table block; returns its size.
  size_t table_layout(size_t off[3]) const {
    const int sc = u.sphere_count, lc = u.light_count, all = u.all_spheres_count;
    const int nb = all - sc, ns = all - sc - lc;
    off[0] = (size_t)(sc > 0 ? sc : 1) * sizeof(sfrt::GlslWall);
    off[1] = off[0] + (size_t)(nb > 0 ? nb : 1) * sizeof(sfrt::GlslBall);
    off[2] = off[1] + (size_t)(lc * ns > 0 ? lc * ns : 1) * sizeof(sfrt::GlslPair);
    return off[2] + (size_t)sfrt::kGlslMax * sizeof(sfrt::GlslMat);
  }

  // The table block walls | balls | pairs | mats at blob (table_layout's offsets) for the cameras
  // at cams[0 .. ncams): scene terms but for GlslPair::cos_lit, whose shortcut is proved for
  // positions near the ball and so is kept only where EVERY camera is within 1000 of it (a draw:
  // the shader's campos alone; a view batch: all its views -- the shortcut is exact where it
  // applies and -2 switches it off, so a pair that loses it shades the same bytes).
  void build_tables(uint8_t* blob, const size_t off[3], const std::vector<sfrt::GlslWall>& walls,
                    const float (*cams)[3], int ncams) const {
    const sfrt_glsl_uniforms& v = u;
    const int sc = v.sphere_count, lc = v.light_count, all = v.all_spheres_count;
    const int nb = all - sc, ns = all - sc - lc;
    std::vector<sfrt::GlslBall> balls(nb > 0 ? nb : 1);
    for (int k = 0; k < nb; k++) {
      const float* S = v.spheres[sc + k];
      // r_skip: r * (1 + 6e-6) rounded up, the dominance test's inflated radius (glsl_trace.hip
      // kThrMul); NaN for r < 0 or NaN, so such a ball is never skipped
      const float rs = S[3] >= 0.0f ? std::nextafter(S[3] * 0x1.000065p+0f, INFINITY) : NAN;
      balls[k] = {S[0], S[1], S[2], S[3], rs, 0.0f, 0.0f, 0.0f};
    }
    std::vector<sfrt::GlslPair> pairs(lc * ns > 0 ? lc * ns : 1);
    for (int li = 0; li < lc; li++)
      for (int k = 0; k < ns; k++) {
        const float* A = v.spheres[sc + li];
        const float* B = v.spheres[sc + lc + k];
        const float qx = A[0] - B[0], qy = A[1] - B[1], qz = A[2] - B[2];
        const float dist = std::sqrt((qx * qx + qy * qy) + qz * qz);    // distance (:140)
        sfrt::GlslPair& P = pairs[li * ns + k];
        P.dist = dist;
        P.sanglet = sfrt_math::atan2f(B[3], dist);                       // :141
        P.ux = (B[0] - A[0]) / dist;                                     // :142
        P.uy = (B[1] - A[1]) / dist;
        P.uz = (B[2] - A[2]) / dist;
        P.bx = B[0];
        P.by = B[1];
        P.bz = B[2];
        // acos(dot) >= sanglet * (1 + 1e-3) + 1e-3 suffices for a factor of 1
        // (DESIGN.md 5c); only for balls near the camera (|pos - ball| < 2000).
        bool near = true;
        for (int q = 0; q < ncams; q++) {
          const float cx = cams[q][0] - B[0], cy = cams[q][1] - B[1], cz = cams[q][2] - B[2];
          const float dcam = std::sqrt((cx * cx + cy * cy) + cz * cz);
          near = near && dcam < 1000.0f;
        }
        P.cos_lit = (P.sanglet > 0.0f && P.sanglet < 1.0f && near)
                        ? std::cos(P.sanglet * 1.001f + 1e-3f) : -2.0f;
      }
    std::vector<sfrt::GlslMat> mats(sfrt::kGlslMax);
    for (int k = 0; k < sfrt::kGlslMax; k++) {
      sfrt::GlslMat& M = mats[k];
      std::memcpy(M.uv, v.uvs[k], sizeof M.uv);
      std::memcpy(M.light, v.lights[k], sizeof M.light);
      M.cx = v.spheres[k][0];
      M.cy = v.spheres[k][1];
      M.cz = v.spheres[k][2];
      M.pad = 0.0f;
    }
    std::memcpy(blob, walls.data(), walls.size() * sizeof walls[0]);
    std::memcpy(blob + off[0], balls.data(), balls.size() * sizeof balls[0]);
    std::memcpy(blob + off[1], pairs.data(), pairs.size() * sizeof pairs[0]);
    std::memcpy(blob + off[2], mats.data(), mats.size() * sizeof mats[0]);
  }

  // Frame record + per-draw tables on stream s (stream-ordered reuse).  frame false: for a ray
  // batch that reads neither the view uniforms nor (textured false) the ground.
  int prepare(sfrt::GlslFrame& f, hipStream_t s, bool frame = true, bool textured = true) {
    if (textured && !d_mip) return SFRT_E_NO_TEXTURE;
    int rc = validate(frame);
    if (rc) return rc;
    HIP_TRY(ground.before_read(s));  // a set_ground queued on another stream lands first
    std::memset(&f, 0, sizeof f);
    const sfrt_glsl_uniforms& v = u;
    const std::vector<sfrt::GlslWall> walls = wall_table();
    camera_terms(v.campos, v.rotation, v.fov, frame, walls, f);
    f.ss = ss;
    f.sc = v.sphere_count;
    f.lc = v.light_count;
    f.all = v.all_spheres_count;
    if (staged_version == u_version && cur_slot >= 0) {  // launched() re-marks the slot
      HIP_TRY(slots[cur_slot].use_on(s));  // staged, or last read, on another stream: wait for it
      fill_tables(f, slots[cur_slot].d.ptr<uint8_t>(), staged_off);
      return SFRT_OK;
    }
    size_t off[3];
    const size_t bytes = table_layout(off);
    sfrt::TableSlot& t = slots[next_slot];
    HIP_TRY(t.reclaim());
    HIP_TRY(t.grow(bytes, s));  // no wait on other streams (sfrt_host.h)
    uint8_t* blob = t.h.ptr<uint8_t>();
    build_tables(blob, off, walls, &v.campos, 1);
    HIP_TRY(hipMemcpyAsync(t.d.ptr(), blob, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(t.staged(s));
    cur_slot = next_slot;
    next_slot = (next_slot + 1) % kSlots;
    staged_version = u_version;
    for (int k = 0; k < 3; k++) staged_off[k] = off[k];
    fill_tables(f, t.d.ptr<uint8_t>(), staged_off);
    return SFRT_OK;
  }

  // The frame record's device pointers: the staged tables at base, the ground's mip chain.
  void fill_tables(sfrt::GlslFrame& f, uint8_t* base, const size_t* off) {
    f.walls = (const sfrt::GlslWall*)base;
    f.balls = (const sfrt::GlslBall*)(base + off[0]);
    f.pairs = (const sfrt::GlslPair*)(base + off[1]);
    f.mats = (const sfrt::GlslMat*)(base + off[2]);
    f.mip = d_mip;
    f.mip_levels = mip_levels;
    for (int k = 0; k < sfrt::kGlslMipLevels; k++) {
      f.mip_w[k] = mip_w[k];
      f.mip_h[k] = mip_h[k];
      f.mip_off[k] = mip_off[k];
    }
    f.status = d_status;
  }

  // The current table slot's event, for the launch that reads it to record (its stop event:
  // sfrt_host.h TableSlot::launch_event), and the slot marked busy once that launch is queued.
  void* launch_event() const { return slots[cur_slot].launch_event(); }
  hipError_t launched(hipStream_t s) { return slots[cur_slot].launched_with(s); }

  int read_status(hipStream_t s) {
    int st = 0;
    HIP_TRY(sfrt::read_status(d_status, s, &st));
    return (st & 1) ? SFRT_E_MARCH_LIMIT : SFRT_OK;
  }
};

namespace {

// "spheres[12]" -> ("spheres", 12); plain names -> index -1.
bool parse_name(const char* name, char* base, size_t cap, int* index) {
  const char* br = std::strchr(name, '[');
  size_t n = br ? (size_t)(br - name) : std::strlen(name);
  if (n == 0 || n >= cap) return false;
  std::memcpy(base, name, n);
  base[n] = 0;
  *index = -1;
  if (br) {
    char* end = nullptr;
    const long k = std::strtol(br + 1, &end, 10);
    if (end == br + 1 || *end != ']' || end[1] != 0 || k < 0 || k >= SFRT_GLSL_MAX_SPHERES)
      return false;
    *index = (int)k;
  }
  return true;
}

}  // namespace

extern "C" {

int sfrt_glsl_create(int hip_device, sfrt_glsl** out) {
  if (!out) return SFRT_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || hip_device < 0 || hip_device >= count)
    return SFRT_E_HIP;
  sfrt_glsl* g = new sfrt_glsl();
  g->device = hip_device;
  sfrt::DeviceGuard dg(hip_device);
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&g->d_status, sizeof(int)) != hipSuccess ||
      hipMemset(g->d_status, 0, sizeof(int)) != hipSuccess) {
    delete g;
    return SFRT_E_HIP;
  }
  *out = g;
  return SFRT_OK;
}

void sfrt_glsl_destroy(sfrt_glsl* g) { delete g; }

int sfrt_glsl_set_ground(sfrt_glsl* g, const uint8_t* rgba, int w, int h) {
  if (!g || !rgba || !pow2(w) || !pow2(h) || w > 32768 || h > 32768) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  std::vector<uint32_t> chain;
  int lw[sfrt::kGlslMipLevels], lh[sfrt::kGlslMipLevels], off[sfrt::kGlslMipLevels], levels = 0;
  build_mips(rgba, w, h, chain, lw, lh, off, &levels);
  sfrt::DeviceGuard dg(g->device);
  // Stream-ordered, no device-wide wait: the new chain goes up on the object's stream behind every
  // draw that read the old one (device-side waits on the table slots' events, sfrt::SharedBuffer)
  // and the old chain is freed in that order; draws on other streams wait for the upload.
  const size_t bytes = chain.size() * 4;
  void* staged = nullptr;
  HIP_TRY(g->mip_stage.fill(chain.data(), bytes, &staged));
  HIP_TRY(g->ground.before_write(g->stream, g->slots));
  uint32_t* chain_d = nullptr;
  HIP_TRY(hipMallocAsync((void**)&chain_d, bytes, g->stream));
  HIP_TRY(hipMemcpyAsync(chain_d, staged, bytes, hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g->mip_stage.copied(g->stream));
  if (g->d_mip) HIP_TRY(hipFreeAsync(g->d_mip, g->stream));
  g->d_mip = chain_d;
  HIP_TRY(g->ground.after_write(g->stream));
  g->mip_levels = levels;
  for (int k = 0; k < sfrt::kGlslMipLevels; k++) {
    g->mip_w[k] = k < levels ? lw[k] : 0;
    g->mip_h[k] = k < levels ? lh[k] : 0;
    g->mip_off[k] = k < levels ? off[k] : 0;
  }
  g->ground_w = w;
  g->ground_h = h;
  return SFRT_OK;
}

int sfrt_glsl_set_uniforms(sfrt_glsl* g, const sfrt_glsl_uniforms* u) {
  if (!g || !u) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  g->u = *u;
  g->u_version++;
  return SFRT_OK;
}

int sfrt_glsl_get_uniforms(sfrt_glsl* g, sfrt_glsl_uniforms* u) {
  if (!g || !u) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  *u = g->u;
  return SFRT_OK;
}

int sfrt_glsl_set_uniform(sfrt_glsl* g, const char* name, const float* v, int n) {
  if (!g || !name || !v || n < 1 || n > 4) return SFRT_E_INVALID;
  char base[32];
  int k;
  if (!parse_name(name, base, sizeof base, &k)) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  sfrt_glsl_uniforms& u = g->u;
  float* dst = nullptr;
  int want = 0;
  if (k < 0) {
    if (!std::strcmp(base, "campos")) dst = u.campos, want = 3;
    else if (!std::strcmp(base, "rotation")) dst = u.rotation, want = 2;
    else if (!std::strcmp(base, "fov")) dst = u.fov, want = 2;
    else if (!std::strcmp(base, "size")) dst = u.size, want = 2;
  } else {
    if (!std::strcmp(base, "spheres")) dst = u.spheres[k], want = 4;
    else if (!std::strcmp(base, "uvs")) dst = u.uvs[k], want = 4;
    else if (!std::strcmp(base, "lights")) dst = u.lights[k], want = 4;
  }
  if (!dst || n != want) return SFRT_E_INVALID;
  std::memcpy(dst, v, sizeof(float) * n);
  g->u_version++;
  return SFRT_OK;
}

int sfrt_glsl_set_uniform_int(sfrt_glsl* g, const char* name, int value) {
  if (!g || !name) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  if (!std::strcmp(name, "sphereCount")) g->u.sphere_count = value;
  else if (!std::strcmp(name, "allSpheresCount")) g->u.all_spheres_count = value;
  else if (!std::strcmp(name, "lightCount")) g->u.light_count = value;
  else return SFRT_E_INVALID;
  g->u_version++;
  return SFRT_OK;
}

}  // extern "C"

// sfrt_glsl_draw and sfrt_glsl_draw_aux (with_aux false for the plain call).
static int draw_body(sfrt_glsl* g, void* dev_pixels, int width, int height, int64_t pitch_bytes,
                     const sfrt_aux_planes* aux, bool with_aux, int row0, int rows,
                     void* hip_stream) {
  if (!g || !dev_pixels || width <= 0 || height <= 0 || row0 < 0 || rows < 0 ||
      row0 + rows > height || pitch_bytes < (int64_t)width * 4 || pitch_bytes % 4 != 0 ||
      height >= (1 << 24) || width >= (1 << 24))
    return SFRT_E_INVALID;
  sfrt::GlslAux a{};
  if (with_aux) {
    if (!aux || (!aux->depth && !aux->sphere && !aux->steps)) return SFRT_E_INVALID;
    if (!sfrt::aux_plane(aux->depth, aux->depth_pitch_bytes, width, a.depth, a.depth_pitch) ||
        !sfrt::aux_plane(aux->sphere, aux->sphere_pitch_bytes, width, a.sphere, a.sphere_pitch) ||
        !sfrt::aux_plane(aux->steps, aux->steps_pitch_bytes, width, a.steps, a.steps_pitch))
      return SFRT_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  // supersampled: the fragments of the S * width x S * height target, gl_FragCoord exact below 2^24
  const int ss = g->ss;
  if ((height << ss) >= (1 << 24) || (width << ss) >= (1 << 24)) return SFRT_E_INVALID;
  sfrt::DeviceGuard dg(g->device);
  hipStream_t s = (hipStream_t)hip_stream;
  sfrt::GlslFrame f;
  if (rows == 0) return SFRT_OK;
  const int rc = g->prepare(f, s);
  if (rc) return rc;
  f.width = width << ss;
  f.height = height << ss;
  f.row0 = row0 << ss;
  f.rows = rows << ss;
  f.tiles_x = (f.width + 7) / 8;
  f.out = (uint32_t*)dev_pixels;
  f.out_pitch = pitch_bytes / 4;
  long long tiles = 0;
  // the same key with and without planes: an aux draw and a plain draw of one stream share a chain
  const long long key = g->tile_order_on ? sfrt::glsl_tile_key(f, &tiles) : 0;
  sfrt::TileSchedPtrs p;
  sfrt::TileSched& sched = g->scheds.chain[g->scheds.pick(s)];
  HIP_TRY(sched.begin(key, tiles, s, g->tile_order_on, p));
  p.link(f);
  const bool queued = sfrt::launch_glsl(f, s, g->launch_event(), with_aux ? &a : nullptr) == 0;
  HIP_TRY(sched.end(p, s, queued));
  if (!queued) return SFRT_E_HIP;
  HIP_TRY(g->launched(s));
  return SFRT_OK;
}

// sfrt_glsl_draw_image and sfrt_glsl_draw_image_aux (planes null for the plain call): depth,
// sphere, steps, host planes of width * height elements.
static int draw_image_body(sfrt_glsl* g, uint8_t* pixels, void* const* planes, int width, int height) {
  if (!g || !pixels || width <= 0 || height <= 0 || height >= (1 << 24) || width >= (1 << 24))
    return SFRT_E_INVALID;
  if (planes && !planes[0] && !planes[1] && !planes[2]) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  const int ss = g->ss;  // supersampled: the sample grid; d_frame and the copy stay width x height
  if ((height << ss) >= (1 << 24) || (width << ss) >= (1 << 24)) return SFRT_E_INVALID;
  sfrt::DeviceGuard dg(g->device);
  const size_t px = (size_t)width * height;
  // stream-ordered behind the last draw_image on the object's stream
  HIP_TRY(g->d_frame.reserve(px * 4, g->stream));
  for (int q = 0; planes && q < 3; q++)  // compact planes beside the compact frame
    if (planes[q]) HIP_TRY(g->d_aux[q].reserve(px * 4, g->stream));
  sfrt::GlslAux a{};
  if (planes) {
    a.depth = planes[0] ? g->d_aux[0].ptr<float>() : nullptr;
    a.sphere = planes[1] ? g->d_aux[1].ptr<int32_t>() : nullptr;
    a.steps = planes[2] ? g->d_aux[2].ptr<int32_t>() : nullptr;
    a.depth_pitch = a.sphere_pitch = a.steps_pitch = width;
  }
  sfrt::GlslFrame f;
  int rc = g->prepare(f, g->stream);
  if (rc) return rc;
  f.width = width << ss;
  f.height = height << ss;
  f.row0 = 0;
  f.rows = f.height;
  f.tiles_x = (f.width + 7) / 8;
  f.out = g->d_frame.ptr<uint32_t>();
  f.out_pitch = width;
  if (sfrt::launch_glsl(f, g->stream, g->launch_event(), planes ? &a : nullptr)) return SFRT_E_HIP;
  HIP_TRY(g->launched(g->stream));
  HIP_TRY(hipMemcpyAsync(pixels, g->d_frame.ptr(), px * 4, hipMemcpyDeviceToHost, g->stream));
  for (int q = 0; planes && q < 3; q++)
    if (planes[q])
      HIP_TRY(hipMemcpyAsync(planes[q], g->d_aux[q].ptr(), px * 4, hipMemcpyDeviceToHost, g->stream));
  return g->read_status(g->stream);
}

// sfrt_glsl_render_views and sfrt_glsl_render_views_aux (with_aux false for the plain call): view k
// is the whole frame that setUniform(campos, rotation, fov of views[k].cam) + draw[_aux] would
// write, all views in one launch of the view kernels (glsl_trace.h launch_glsl_views).  The
// per-camera part of a draw's frame record is built per view by the function prepare() builds the
// draw's with (camera_terms), into one pinned block
//   count view records | walls | balls | pairs | mats
// (the table block 16-byte aligned; its pairs keep the lit shortcut only where every view of the
// batch may have it, build_tables), sent by one copy on the caller's stream from a slot of the view
// ring.  Nothing of the shader is written: not its uniforms or u_version, not the draws' staged
// slot or staged_version, not the tile chains.
static int render_views_body(sfrt_glsl* g, const sfrt_view* views, const sfrt_aux_planes* planes,
                             bool with_aux, int count, int width, int height, int64_t pitch_bytes,
                             int flags, void* hip_stream) {
  if (!g || !views || count < 0 || count > SFRT_MAX_VIEWS || flags != 0 || width <= 0 ||
      height <= 0 || height >= (1 << 24) || width >= (1 << 24) || pitch_bytes % 4 != 0 ||
      pitch_bytes < (int64_t)width * 4 || (with_aux && !planes))
    return SFRT_E_INVALID;
  std::vector<sfrt::GlslAux> aux(with_aux ? (size_t)count : 0);
  for (int k = 0; k < count; k++) {
    const sfrt_camera& c = views[k].cam;
    const float rotation[2] = {c.rotation, c.hrotation}, fov[2] = {c.fov_h, c.fov_v};
    if (!views[k].dev_pixels || !sfrt::aligned4({views[k].dev_pixels}) ||
        !sfrt_glsl::camera_ok(c.pos, rotation, fov))
      return SFRT_E_INVALID;
    if (!with_aux) continue;
    const sfrt_aux_planes& p = planes[k];
    sfrt::GlslAux& a = aux[(size_t)k];
    if ((!p.depth && !p.sphere && !p.steps) ||
        !sfrt::aux_plane(p.depth, p.depth_pitch_bytes, width, a.depth, a.depth_pitch) ||
        !sfrt::aux_plane(p.sphere, p.sphere_pitch_bytes, width, a.sphere, a.sphere_pitch) ||
        !sfrt::aux_plane(p.steps, p.steps_pitch_bytes, width, a.steps, a.steps_pitch))
      return SFRT_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  if (count == 0) return SFRT_OK;
  const int ss = g->ss;
  if ((height << ss) >= (1 << 24) || (width << ss) >= (1 << 24)) return SFRT_E_INVALID;
  if (!g->d_mip) return SFRT_E_NO_TEXTURE;
  const int rc = g->validate(true, false);  // the scene uniforms and `size`; the cameras: above
  if (rc) return rc;
  // The frame geometry of a whole-frame draw, the same for every view, and the grid it gives,
  // refused before anything is queued if one launch cannot take it.
  sfrt::GlslFrame f;
  std::memset(&f, 0, sizeof f);
  f.ss = ss;
  f.sc = g->u.sphere_count;
  f.lc = g->u.light_count;
  f.all = g->u.all_spheres_count;
  f.width = width << ss;
  f.height = height << ss;
  f.row0 = 0;
  f.rows = f.height;
  f.tiles_x = (f.width + 7) / 8;
  f.out_pitch = pitch_bytes / 4;
  if (!sfrt::glsl_views_grid_ok(f, count)) return SFRT_E_INVALID;
  sfrt::DeviceGuard dg(g->device);
  hipStream_t s = (hipStream_t)hip_stream;
  HIP_TRY(g->ground.before_read(s));  // a set_ground queued on another stream lands first
  size_t off[3];
  const size_t at_tables = ((size_t)count * sizeof(sfrt::GlslViewRec) + 15) / 16 * 16;
  const size_t bytes = at_tables + g->table_layout(off);
  sfrt::TableSlot& t = g->slots[sfrt_glsl::kSlots + g->next_view_slot];
  g->next_view_slot = (g->next_view_slot + 1) % sfrt_glsl::kViewSlots;
  HIP_TRY(t.reclaim());  // the launch that read the slot's last block is done (no device-wide wait)
  HIP_TRY(t.grow(bytes, s));
  uint8_t* const h = t.h.ptr<uint8_t>();
  uint8_t* const d = t.d.ptr<uint8_t>();
  const std::vector<sfrt::GlslWall> walls = g->wall_table();
  std::vector<float> cams((size_t)count * 3);
  for (int k = 0; k < count; k++) {
    const sfrt_camera& c = views[k].cam;
    const float rotation[2] = {c.rotation, c.hrotation}, fov[2] = {c.fov_h, c.fov_v};
    sfrt::GlslViewRec r;
    std::memset(&r, 0, sizeof r);
    g->camera_terms(c.pos, rotation, fov, true, walls, r);
    r.out = (uint32_t*)views[k].dev_pixels;
    if (with_aux) r.aux = aux[(size_t)k];
    std::memcpy(h + (size_t)k * sizeof r, &r, sizeof r);
    for (int q = 0; q < 3; q++) cams[(size_t)k * 3 + q] = c.pos[q];
  }
  g->build_tables(h + at_tables, off, walls, (const float(*)[3])cams.data(), count);
  HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  // the copy is queued: on a failure below the slot stays busy until it has run
  g->fill_tables(f, d + at_tables, off);
  if (sfrt::launch_glsl_views(f, (const sfrt::GlslViewRec*)d, count, with_aux, s, t.launch_event())) {
    (void)t.staged(s);
    return SFRT_E_HIP;
  }
  HIP_TRY(t.launched_with(s));
  return SFRT_OK;
}

// ---- batched ray queries (include/sfrt.h) ----
namespace {

// One launch of the ray-batch kernel on s with the shader's mutex held: the draw's snapshot of the
// uniforms (prepare: the staged tables, the per-campos host terms) and nothing of the view, the
// options or the tile-order chains.
int cast_rays_launch(sfrt_glsl* g, const float* dev_dirs, int64_t count, const sfrt_ray_hits& out,
                     hipStream_t s) {
  sfrt::GlslFrame f;
  const int rc = g->prepare(f, s, false, out.rgba != nullptr);
  if (rc) return rc;
  sfrt::GlslRays a{};
  a.dirs = dev_dirs;
  a.count = count;
  a.pos = out.pos;
  a.depth = out.depth;
  a.sphere = out.sphere;
  a.steps = out.steps;
  a.rgba = (uint32_t*)out.rgba;
  if (sfrt::launch_glsl_rays(f, a, s, g->launch_event())) return SFRT_E_HIP;
  HIP_TRY(g->launched(s));
  return SFRT_OK;
}

}  // namespace

extern "C" {

int sfrt_glsl_draw(sfrt_glsl* g, void* dev_pixels, int width, int height, int64_t pitch_bytes,
                   int row0, int rows, void* hip_stream) {
  return draw_body(g, dev_pixels, width, height, pitch_bytes, nullptr, false, row0, rows, hip_stream);
}

int sfrt_glsl_draw_aux(sfrt_glsl* g, void* dev_pixels, int width, int height, int64_t pitch_bytes,
                       const sfrt_aux_planes* aux, int row0, int rows, void* hip_stream) {
  return draw_body(g, dev_pixels, width, height, pitch_bytes, aux, true, row0, rows, hip_stream);
}

int sfrt_glsl_draw_image(sfrt_glsl* g, uint8_t* pixels, int width, int height) {
  return draw_image_body(g, pixels, nullptr, width, height);
}

int sfrt_glsl_draw_image_aux(sfrt_glsl* g, uint8_t* pixels, float* depth, int32_t* sphere,
                             int32_t* steps, int width, int height) {
  void* const planes[3] = {depth, sphere, steps};
  return draw_image_body(g, pixels, planes, width, height);
}

int sfrt_glsl_render_views(sfrt_glsl* g, const sfrt_view* views, int count, int width, int height,
                           int64_t pitch_bytes, int flags, void* hip_stream) {
  return render_views_body(g, views, nullptr, false, count, width, height, pitch_bytes, flags,
                           hip_stream);
}

int sfrt_glsl_render_views_aux(sfrt_glsl* g, const sfrt_view* views, const sfrt_aux_planes* planes,
                               int count, int width, int height, int64_t pitch_bytes, int flags,
                               void* hip_stream) {
  return render_views_body(g, views, planes, true, count, width, height, pitch_bytes, flags,
                           hip_stream);
}

int sfrt_glsl_cast_rays_device(sfrt_glsl* g, const float* dev_dirs, int64_t count,
                               const sfrt_ray_hits* dev_out, void* hip_stream) {
  const int rc = sfrt::ray_hits_args(g, dev_dirs, nullptr, count, dev_out);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g->mu);
  if (count == 0) return SFRT_OK;
  sfrt::DeviceGuard dg(g->device);
  return cast_rays_launch(g, dev_dirs, count, *dev_out, (hipStream_t)hip_stream);
}

int sfrt_glsl_cast_rays(sfrt_glsl* g, const float* dirs, int64_t count, const sfrt_ray_hits* out) {
  int rc = sfrt::ray_hits_args(g, dirs, nullptr, count, out);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g->mu);
  if (count == 0) return SFRT_OK;
  if (out->rgba && !g->d_mip) return SFRT_E_NO_TEXTURE;  // before anything is staged
  if ((rc = g->validate(false))) return rc;
  sfrt::DeviceGuard dg(g->device);
  // The layout only: one device buffer on the object's stream (the last host call waited for its
  // own copies), copied straight from and to the caller's memory.
  const sfrt::BatchLayout l((size_t)count, {{dirs, 12}},
                            {{out->pos, 12}, {out->depth, 4}, {out->sphere, 4}, {out->steps, 4},
                             {out->rgba, 4}});
  HIP_TRY(g->d_rays.reserve(l.bytes, g->stream));
  void* const d = g->d_rays.ptr();
  HIP_TRY(hipMemcpyAsync(d, dirs, l.in_bytes, hipMemcpyHostToDevice, g->stream));
  const sfrt_ray_hits dev{l.out_at<float>(d, 0), l.out_at<float>(d, 1), l.out_at<int32_t>(d, 2),
                          l.out_at<int32_t>(d, 3), l.out_at<uint8_t>(d, 4)};
  if ((rc = cast_rays_launch(g, l.in_at<float>(d, 0), count, dev, g->stream))) return rc;
  for (int q = 0; q < l.n_out; q++)
    if (l.out[q].host)
      HIP_TRY(hipMemcpyAsync((void*)l.out[q].host, l.out_at<uint8_t>(d, q), l.n * l.out[q].elem,
                             hipMemcpyDeviceToHost, g->stream));
  return g->read_status(g->stream);  // SFRT_E_MARCH_LIMIT: the outputs are written, as draw_image's
}

int sfrt_glsl_set_option(sfrt_glsl* g, int option, int value) {
  if (!g) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  if (option == SFRT_OPT_TILE_ORDER) {
    g->tile_order_on = value == 2 ? 2 : value ? 1 : 0;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_SUPERSAMPLE) {
    if (value != 1 && value != 2 && value != 4) return SFRT_E_INVALID;
    const int ss = value == 4 ? 2 : value == 2 ? 1 : 0;
    if (ss != g->ss) g->u_version++;  // the next draw stages its tables afresh
    g->ss = ss;
    return SFRT_OK;
  }
  return SFRT_E_INVALID;
}

int sfrt_glsl_get_option(const sfrt_glsl* g, int option, int* value) {
  if (!g || !value) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  switch (option) {
    case SFRT_OPT_TILE_ORDER: *value = g->tile_order_on; return SFRT_OK;
    case SFRT_OPT_SUPERSAMPLE: *value = 1 << g->ss; return SFRT_OK;
    default: return SFRT_E_INVALID;
  }
}

int sfrt_glsl_check(sfrt_glsl* g, void* hip_stream) {
  if (!g) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  sfrt::DeviceGuard dg(g->device);
  return g->read_status((hipStream_t)hip_stream);
}

}  // extern "C"
