// sfrt_world.cpp -- host side of the drop-in: a C++ mirror of the scene state
// that SphereWorld::UpdateImage reads, the per-frame preparation the kernel
// needs, and the extern "C" boundary declared in include/sfrt.h.
//
// Reference interface mirrored (paths under /root/reference/Raytracing/):
//   SphereWorld::width/height/cam     SphereWorld.h:50-52 (defaults 320x180, fov 75/47 deg)
//   SphereWorld::SphereWorld          SphereWorld.cpp:43-77 (fov -> radians :72-73)
//   SphereWorld::AddSphere            SphereWorld.cpp:177-190
//   SphereWorld::UpdateSpheres (sort) SphereWorld.cpp:199-212
//   SphereWorld::UpdateImage          SphereWorld.cpp:83-112
//   textures[0]                       SphereWorld.h:74, SphereWorld.cpp:52
// Compiled with -ffp-contract=off: every float expression below is
// evaluated exactly as the reference writes it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "sfrt.h"
#include "sfrt_host.h"
#include "sfrt_math.h"
#include "sfrt_raycache.h"
#include "sfrt_sched.h"
#include "sfrt_trace.h"

#pragma clang fp contract(off)


namespace {

constexpr float kPI = 3.1415926535f;  // SphereWorld.h:6

struct V3 {
  float x, y, z;
};
inline V3 vsub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// SphereWorld.cpp:340-343
inline float vlength(V3 v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
// SphereWorld.cpp:27-31
inline V3 rot_x(V3 v, float amount) {
  const float s = std::sin(amount);
  const float c = std::cos(amount);
  return {v.x, v.y * c - v.z * s, v.y * s + v.z * c};
}
// SphereWorld.cpp:32-36
inline V3 rot_y(V3 v, float amount) {
  const float s = std::sin(amount);
  const float c = std::cos(amount);
  return {v.x * c + v.z * s, v.y, -v.x * s + v.z * c};
}
inline V3 center(const sfrt_sphere& s) { return {s.x, s.y, s.z}; }

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
// A camera sfrt_world_set_camera takes.
bool camera_ok(const sfrt_camera& c) {
  return finite3(c.pos) && std::isfinite(c.rotation) && std::isfinite(c.hrotation) &&
         std::isfinite(c.fov_h) && std::isfinite(c.fov_v);
}
bool sphere_ok(const sfrt_sphere& s) {
  return std::isfinite(s.x) && std::isfinite(s.y) && std::isfinite(s.z) && std::isfinite(s.radius) &&
         s.radius > 0.0f;
}

// Stable insertion by |c - cam| + r, inserted after equal keys (SphereWorld.cpp:201-212).
// Returns the permutation (new position -> old index).
std::vector<size_t> sort_spheres(std::vector<sfrt_sphere>& spheres, V3 cam) {
  std::vector<sfrt_sphere> temp = spheres;
  std::vector<size_t> order;
  spheres.clear();
  for (size_t k = 0; k < temp.size(); k++) {
    const sfrt_sphere& t = temp[k];
    const float dist = vlength(vsub(center(t), cam)) + t.radius;
    size_t ins = 0;
    for (size_t j = 0; j < spheres.size(); j++) {
      if (dist < vlength(vsub(center(spheres[j]), cam)) + spheres[j].radius) break;
      ins++;
    }
    spheres.insert(spheres.begin() + (long)ins, t);
    order.insert(order.begin() + (long)ins, k);
  }
  return order;
}

template <class T>
void permute(std::vector<T>& v, const std::vector<size_t>& order) {
  std::vector<T> out(order.size());
  for (size_t i = 0; i < order.size(); i++) out[i] = v[order[i]];
  v.swap(out);
}

bool passes(float r, float s) { return r - std::sqrt(s) > 0.01f; }  // SphereWorld.cpp:365-366

// Smallest binary32 s >= 0 for which the reference test fails; the test is
// monotone in s (sqrtf and the subtraction are monotone), so
// passes(r, s) <=> s < threshold for every s >= 0 (and NaN s fails both).
float pass_threshold(float r) {
  if (!passes(r, 0.0f)) return 0.0f;
  uint32_t lo = 0, hi = 0x7f800000u;  // passes(lo), !passes(hi = +inf)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    float s;
    std::memcpy(&s, &mid, 4);
    if (passes(r, s)) lo = mid; else hi = mid;
  }
  float t;
  std::memcpy(&t, &hi, 4);
  return t;
}

}  // namespace

struct sfrt_world {
  int device = 0;
  // --- SphereWorld state read by UpdateImage ---
  int width = 320;   // SphereWorld.h:50
  int height = 180;  // SphereWorld.h:51
  sfrt_camera cam{};
  std::vector<sfrt_sphere> spheres;
  // Per-sphere texture slot, parallel to `spheres` (the "all textures" extension
  // of SURVEY 8d config 3; 0 everywhere = the reference, textures[0]).
  std::vector<int32_t> sphere_tex;
  std::vector<uint8_t> tex_host[SFRT_TEXTURE_SLOTS];
  int tex_w[SFRT_TEXTURE_SLOTS] = {};
  int tex_h[SFRT_TEXTURE_SLOTS] = {};
  bool tex_alpha01[SFRT_TEXTURE_SLOTS] = {};  // every texel's alpha is 0 or 255
  int tex_alpha_one[SFRT_TEXTURE_SLOTS] = {};  // the alpha every texel has, or -1
  uint32_t tex_off[SFRT_TEXTURE_SLOTS] = {};  // texel offset of each slot in the atlas
  int cull = 1;
  int rays = 0;           // SFRT_OPT_RAYS_PER_LANE (0 = automatic)
  int tile_order_on = 1;  // SFRT_OPT_TILE_ORDER
  int ss = 0;             // SFRT_OPT_SUPERSAMPLE: log2 of the factor S (0, 1, 2)
  int ray_cache_mb = 512;  // SFRT_OPT_RAY_CACHE_MB: MiB of ray caches over all chains (0: off)
  int hit_cache_mb = 512;  // SFRT_OPT_HIT_CACHE_MB: MB (10^6 bytes) of hit caches over all chains (0: off)
  int texel_cache = 1;     // SFRT_OPT_TEXEL_CACHE: the texel layer on the hit cache, under its budget (0: off)
  // SFRT_OPT_COMPACT_TEXELS: the compact layer on the texel cache (0: off; 1: launches at four pixels
  // per lane whose records travel in the arguments, the shape it was proven at; 2: every eligible one)
  int compact_texels = 1;
  // SFRT_OPT_PIXEL_CACHE: the pixel layer on top of the chain's other layers (0: off; 1: launches
  // that are not supersampled, carry their records in the arguments and draw from an atlas the compact
  // layer can index, the shapes it was proven at; 2: every plain render_band launch)
  int pixel_cache = 1;
  // Every write of the atlas (sfrt_world_load_texture, the only one) counts here: the pixel layer's
  // key holds it (sfrt_raycache.h PixelKey), no texel's value.
  long long tex_generation = 0;
  // --- device resources ---
  hipStream_t stream = nullptr;
  uint32_t* d_tex = nullptr;  // texture atlas: every loaded slot, back to back
  // the brightness classes' table (sfrt_raycache.h BrightClasses::rep), uploaded when the world is
  // created; kCompactClassLimit entries (null: no memory for it, the compact layer is never filled)
  uint32_t* d_bright_rep = nullptr;
  size_t d_tex_texels = 0;
  // A new texture goes into a new atlas, uploaded on `stream` from pinned staging; launches
  // queued earlier keep reading the old one (its pointer is in their arguments), launches queued
  // later on another stream wait for the upload once (tex_written).  The old atlases are freed
  // once the device has drained anyway (the destructor), or in one sweep per kRetiredTexBytes.
  sfrt::SharedBuffer tex_written;
  sfrt::PinnedStage tex_stage;
  std::vector<void*> retired_tex;
  size_t retired_tex_bytes = 0;
  static constexpr size_t kRetiredTexBytes = 64u << 20;
  int* d_status = nullptr;
  int* d_pixel_status = nullptr;  // the pixel layers' status words, one per chain (caches[])
  sfrt::TileChains scheds;  // adaptive tile order (sfrt_sched.h), one chain per stream
  sfrt::TileSched dump_sched;  // sfrt_world_trace_points' own chain (never the frames')
  int cur_chain = 0;        // the chain of the launch between sched_begin and sched_end
  // The chains' caches (sfrt_raycache.h ChainCaches: directions and tile records, cull cache, hit
  // cache), one per chain like chain_cam[]; a stream that takes a chain over keeps them.  Of the
  // launch between sched_begin and sched_end: what its chain decided, which launch_trace reads
  // (decided == false: the launch takes no part).  Counters: the three sfrt_world_*_cache_stats.
  sfrt::ChainCaches caches[sfrt::TileChains::kChains];
  sfrt::TexKey tex_key;  // sched_begin's scratch (its .cull: the launch's CullKey): the vectors keep their capacity
  sfrt::TraceCaches launch_caches;
  sfrt::CacheCounters cache_stats;
  // Device copies of the sphere records for launches that read them from memory
  // (> 64 spheres, trace_points): a ring of slots, each with pinned staging and
  // the event of the last launch that read it, so a slot is never overwritten
  // while a launch on any stream may still read it.
  static constexpr int kRing = 8;
  sfrt::SphereRec* d_spheres[kRing] = {};
  sfrt::SphereRec* h_spheres[kRing] = {};
  hipEvent_t spheres_ev[kRing] = {};    // relayed (sfrt_host.h Relay): the slot's last reader done
  hipEvent_t spheres_stop[kRing] = {};  // that reader's own stop event, on the caller's stream
  sfrt::Relay relay;
  bool spheres_pending[kRing] = {};
  int d_spheres_cap = 0;
  int ring = 0;
  int staged = -1;  // slot staged for the launch being prepared, or -1
  // The host path (update_image): the compact subset's device buffer, on the world's stream, and
  // its pinned D2H staging (sfrt_host.h DeviceBuf, PinnedBuf).  The same pair per plane of
  // sfrt_world_update_image_aux (depth, sphere, steps), grown by the first call that asks for it.
  sfrt::DeviceBuf d_frame, d_aux[3];
  sfrt::PinnedBuf h_stage, h_aux[3];
  sfrt::BatchStage ray_stage;  // staging of sfrt_world_cast_rays (the host call)
  sfrt::RetiredHost retired_host;  // the record ring's replaced pinned buffers (sfrt_host.h)
  std::vector<void*> retired_device;  // replaced record rings, freed with the world
  // The tables of sfrt_world_render_views (view records and sphere records in one block): a ring
  // of table slots under the record ring's rule (sfrt_host.h TableSlot) -- a slot is restaged only
  // after the launch that read it, on whatever stream, is done (its relayed stop event).
  static constexpr int kViewSlots = kRing;
  sfrt::TableSlot view_slots[kViewSlots];
  int next_view_slot = 0;
  // --- frame pipeline (display path): render k+1 while frame k is copied ---
  struct PipeSlot {
    sfrt::DeviceBuf d_buf;  // the frame, stream-ordered on the world's stream
    hipEvent_t rendered = nullptr, copied = nullptr;
    int* d_status = nullptr;    // this frame's march/texel flags
    int* h_status = nullptr;    // pinned copy, valid once `copied` completes
    bool used = false;
  };
  static constexpr int kPipe = 2;
  PipeSlot pipe[kPipe];
  hipStream_t copy_stream = nullptr;
  int64_t next_ticket = 0;
  mutable std::mutex mu;  // every entry point, getters included (RenderThreads call concurrently)

  ~sfrt_world() {
    sfrt::DeviceGuard g(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    for (PipeSlot& p : pipe) {
      p.d_buf.release();
      (void)hipFree(p.d_status);
      (void)hipHostFree(p.h_status);
      if (p.rendered) (void)hipEventDestroy(p.rendered);
      if (p.copied) (void)hipEventDestroy(p.copied);
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    for (sfrt::ChainCaches& c : caches) c.release_all([](void* p) { return hipFree(p) == hipSuccess; });
    scheds.release();
    dump_sched.release();
    (void)hipFree(d_tex);
    (void)hipFree(d_bright_rep);
    for (void* p : retired_tex) (void)hipFree(p);
    tex_written.release();
    tex_stage.release();
    (void)hipFree(d_status);
    (void)hipFree(d_pixel_status);
    (void)hipDeviceSynchronize();
    for (int k = 0; k < kRing; k++) {
      (void)hipFree(d_spheres[k]);
      (void)hipHostFree(h_spheres[k]);
      if (spheres_ev[k]) (void)hipEventDestroy(spheres_ev[k]);
      if (spheres_stop[k]) (void)hipEventDestroy(spheres_stop[k]);
    }
    relay.release();
    d_frame.release();
    h_stage.release();
    for (int q = 0; q < 3; q++) {
      d_aux[q].release();
      h_aux[q].release();
    }
    ray_stage.release();
    for (sfrt::TableSlot& t : view_slots) t.release();
    retired_host.release();
    for (void* p : retired_device) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int validate() const {
    if (spheres.empty()) return SFRT_E_EMPTY;
    if ((int)spheres.size() > SFRT_MAX_SPHERES) return SFRT_E_TOO_MANY;
    if (tex_host[0].empty() || !d_tex) return SFRT_E_NO_TEXTURE;
    for (int32_t k : sphere_tex)
      if (tex_host[k].empty()) return SFRT_E_NO_TEXTURE;
    if (width <= 0 || height <= 0) return SFRT_E_INVALID;
    // the sample frame's sizes are ints in the kernel (SFRT_OPT_SUPERSAMPLE)
    if (ss && (width > (0x7fffffff >> ss) || height > (0x7fffffff >> ss))) return SFRT_E_INVALID;
    return SFRT_OK;
  }

  // A supersampled frame whose sample grid launch_trace cannot launch is refused before
  // anything is queued (a plain frame that large fails in launch_trace, as it always has).
  int launchable(const sfrt::FrameRec& f) const {
    return f.ss && sfrt::trace_blocks(f) > 0x7fffffffLL ? SFRT_E_INVALID : SFRT_OK;
  }

  // Per-frame records: everything uniform over the frame, computed with the
  // reference's expressions (see sfrt_trace.h).
  // ss_log2 > 0: the frame is the S*width x S*height sample frame (SFRT_OPT_SUPERSAMPLE),
  // i.e. :85-89 are evaluated with those sizes; the caller fills the subset in samples.
  void prepare(sfrt::FrameRec& f, std::vector<sfrt::SphereRec>& recs, int ss_log2 = 0) const {
    prepare_frame(f, cam, spheres, ss_log2);
    prepare_records(recs, spheres, sphere_tex);
  }
  // The frame's part, for any camera and sphere order (the views of sfrt_world_render_views take
  // theirs), and the records' part, for any order and its texture slots.
  void prepare_frame(sfrt::FrameRec& f, const sfrt_camera& cam, const std::vector<sfrt_sphere>& spheres,
                     int ss_log2) const {
    std::memset(&f, 0, sizeof f);
    const int width = this->width << ss_log2, height = this->height << ss_log2;
    f.ss = ss_log2;
    const V3 campos{cam.pos[0], cam.pos[1], cam.pos[2]};
    f.cam[0] = campos.x; f.cam[1] = campos.y; f.cam[2] = campos.z;
    // SphereWorld.cpp:100-104
    V3 up = rot_x({0, -1, 0}, -cam.hrotation);
    V3 forward = rot_x({0, 0, 1}, -cam.hrotation);
    const V3 right = rot_y({1, 0, 0}, cam.rotation);
    forward = rot_y(forward, cam.rotation);
    up = rot_y(up, cam.rotation);
    f.fwd[0] = forward.x; f.fwd[1] = forward.y; f.fwd[2] = forward.z;
    f.right[0] = right.x; f.right[1] = right.y; f.right[2] = right.z;
    f.up[0] = up.x; f.up[1] = up.y; f.up[2] = up.z;
    // SphereWorld.cpp:85-89
    f.v_start = -cam.fov_v;
    f.v_inc = cam.fov_v / height * 2;
    f.h_start = -cam.fov_h;
    f.h_inc = cam.fov_h / width * 2;
    // First march iteration (pos == cam.pos for every pixel), SphereWorld.cpp:362-370.
    float largest = 0.0f;
    int draw = 0;
    for (size_t i = 0; i < spheres.size(); i++) {
      const float dist = vlength(vsub(campos, center(spheres[i])));
      if (spheres[i].radius - dist > 0.01f) {
        const float t = spheres[i].radius - dist;
        largest = largest < t ? t : largest;
        draw = (int)i;
      }
    }
    f.first_l = largest;
    f.first_draw = draw;
    f.n = (int)spheres.size();
    f.width = width;
    f.height = height;
    f.cull = cull;
    f.rays = rays;
    // Culling margin (sphere_trace.hip, cull_mask).  A march step
    // pos += dir * L rounds twice per component, so each step moves the
    // position off the ray's exact line by at most ~2.1e-7 * (|pos| + L) <=
    // 4.2e-7 * R, where R bounds every |coordinate| the march can reach (the
    // camera and every sphere's |c| + r).  Over kCullSafeIterations (1024)
    // steps that is < 4.3e-4 * R, inside the 1e-3 * R margin added to every
    // radius; the reference test additionally needs r - |p - c| > 0.01.
    const V3 origin{0.0f, 0.0f, 0.0f};
    float reach = vlength(campos);
    for (const sfrt_sphere& s : spheres) {
      const float e = vlength(vsub(center(s), origin)) + s.radius;
      reach = reach < e ? e : reach;
    }
    f.cull_margin = 1e-3f * reach + 1e-4f;
    // Non-finite inputs void the drift bound and the cone: visit every sphere.
    bool finite = std::isfinite(f.cull_margin) && std::isfinite(f.first_l) &&
                  std::isfinite(f.h_start) && std::isfinite(f.h_inc) &&
                  std::isfinite(f.v_start) && std::isfinite(f.v_inc);
    for (int q = 0; q < 3; q++)
      finite = finite && std::isfinite(f.cam[q]) && std::isfinite(f.fwd[q]) &&
               std::isfinite(f.right[q]) && std::isfinite(f.up[q]);
    if (!finite) f.cull = 0;
    f.tex = d_tex;
    f.status = d_status;
  }
  void prepare_records(std::vector<sfrt::SphereRec>& recs, const std::vector<sfrt_sphere>& spheres,
                       const std::vector<int32_t>& sphere_tex) const {
    recs.resize(spheres.size());
    for (size_t i = 0; i < spheres.size(); i++) {
      const sfrt_sphere& s = spheres[i];
      sfrt::SphereRec& r = recs[i];
      r.cx = s.x; r.cy = s.y; r.cz = s.z; r.r = s.radius;
      r.s_pass = pass_threshold(s.radius);
      r.atan_c = sfrt_math::atan2f(s.z, s.x);  // == libm atan2f (tests/test_math_exhaustive.py)
      const int k = sphere_tex[i];
      r.tex_off = tex_off[k];
      r.tex_wh = (uint32_t)tex_w[k] | ((uint32_t)tex_h[k] << 16);
    }
  }

  // A larger record ring, waiting for no stream (sfrt_host.h: hipFree / hipHostFree would wait for
  // the whole device): launches queued on any stream may still read the old slots, so the old
  // buffers are retired until the world is destroyed (the ring grows geometrically, and only past
  // the largest sphere count seen); the new ones are plain allocations every stream may use.
  int ensure_sphere_buffers(int n) {
    if (n <= d_spheres_cap) return SFRT_OK;
    const int cap = (int)sfrt::grown_capacity((size_t)d_spheres_cap, (size_t)n);
    for (int k = 0; k < kRing; k++) {
      if (d_spheres[k]) retired_device.push_back(d_spheres[k]);
      retired_host.add(h_spheres[k]);
      d_spheres[k] = nullptr;
      h_spheres[k] = nullptr;
      spheres_pending[k] = false;
    }
    d_spheres_cap = 0;
    for (int k = 0; k < kRing; k++) {
      HIP_TRY(hipMalloc(&d_spheres[k], sizeof(sfrt::SphereRec) * (size_t)cap));
      HIP_TRY(hipHostMalloc(&h_spheres[k], sizeof(sfrt::SphereRec) * (size_t)cap,
                            hipHostMallocDefault));
      if (!spheres_ev[k]) HIP_TRY(hipEventCreateWithFlags(&spheres_ev[k], hipEventDisableTiming));
      if (!spheres_stop[k]) HIP_TRY(hipEventCreateWithFlags(&spheres_stop[k], hipEventDisableTiming));
    }
    d_spheres_cap = cap;
    return SFRT_OK;
  }

  // Upload sphere records when the kernel reads them from device memory.
  int stage_spheres(sfrt::FrameRec& f, const std::vector<sfrt::SphereRec>& recs, hipStream_t s,
                    bool force) {
    staged = -1;
    if (!force && f.n <= sfrt::kInlineSpheres) {
      f.spheres = nullptr;
      return SFRT_OK;
    }
    int rc = ensure_sphere_buffers(f.n);
    if (rc) return rc;
    const int k = ring;
    ring = (ring + 1) % kRing;
    if (spheres_pending[k]) HIP_TRY(hipEventSynchronize(spheres_ev[k]));
    spheres_pending[k] = false;
    std::memcpy(h_spheres[k], recs.data(), sizeof(sfrt::SphereRec) * recs.size());
    HIP_TRY(hipMemcpyAsync(d_spheres[k], h_spheres[k], sizeof(sfrt::SphereRec) * recs.size(),
                           hipMemcpyHostToDevice, s));
    f.spheres = d_spheres[k];
    staged = k;
    return SFRT_OK;
  }

  // After the launch that reads the staged slot has been queued on s.
  int launched(hipStream_t s) {
    if (staged < 0) return SFRT_OK;
    HIP_TRY(relay.record(s, spheres_ev[staged]));
    spheres_pending[staged] = true;
    staged = -1;
    return SFRT_OK;
  }
  // The same through the launch itself: the staged slot's event for launch_trace to record as
  // the kernel's stop event (no marker packet between frames, sfrt_host.h
  // TableSlot::launch_event), then launched_with() once the launch is queued.
  void* ring_event() const { return staged >= 0 ? spheres_stop[staged] : nullptr; }
  int launched_with() {
    if (staged < 0) return SFRT_OK;
    HIP_TRY(relay.pass(spheres_stop[staged], spheres_ev[staged]));
    spheres_pending[staged] = true;
    staged = -1;
    return SFRT_OK;
  }

  // Before a render_band / submit_frame launch on s: link f into the tile-order chain.
  // aux (sfrt_world_render_band_aux): the launch joins the chain like any band but takes no
  // part in the ray cache's policy -- it neither reads, fills nor invalidates the cache, and
  // sched_end commits nothing for it.
  // recs: the launch's records (the cull cache's key holds the fields the cull reads).
  // pixels: a plain render_band launch, the only kind that takes part in the pixel layer.
  int sched_begin(sfrt::FrameRec& f, const std::vector<sfrt::SphereRec>& recs, hipStream_t s,
                  bool aux = false, bool pixels = false) {
    long long tiles = 0;
    const long long key = tile_order_on ? sfrt::trace_tile_key(f, &tiles) : 0;
    sfrt::TileSchedPtrs p;
    cur_chain = scheds.pick(s);
    sfrt::TileSched& sched = scheds.chain[cur_chain];
    const ChainCam& chain_last = chain_cam[cur_chain];
    const long long cap0 = sched.cap;
    HIP_TRY(sched.begin(key, tiles, s, tile_order_on, p));
    if (sched.cap != cap0 && last_fill.chain == cur_chain)
      last_fill.valid = false;  // the cost buffers were reallocated
    p.link(f);
    // a moving camera: the recorded classes are a frame or two off
    f.order_dilate = p.prev_cost && chain_last.valid &&
                     std::memcmp(&chain_last.cam, &cam, sizeof cam) != 0;
    launch_caches = sfrt::TraceCaches{};
    if (!aux && tile_order_on == 1 && p.tile_cost && sched.pending_key != 0) {
      sfrt::CullKey& cull_key = tex_key.cull;
      make_cull_key(cull_key, make_ray_key(f, key), f, recs);
      // The texel layer: every index below the sentinel (load_texture refuses larger atlases;
      // were that to change, the layer is not filled).
      const bool texels = texel_cache != 0 && sfrt::texel_index_fits(d_tex_texels);
      if (texels) make_tex_key(tex_key, recs, f.n);
      sfrt::ChainCaches& mine = caches[cur_chain];
      const int rays = (int)((key >> 56) & 7);
      // The compact layer: the option (1: the shape it was proven at only, DESIGN.md 5 "Compact
      // layer"), no supersampling, every index the records can name in 16 bits, the class table.
      const bool compact_shape = compact_texels == 2 ||
                                 (compact_texels == 1 && rays == 4 && f.n <= sfrt::kInlineSpheres);
      const bool compact = texels && compact_shape && !sfrt::kDiagnosticBuild && d_bright_rep &&
                           sfrt::compact_eligible(recs.data(), f.n, f.ss);
      // The pixel layer: the option, a plain band the copy kernel can address, the status words.
      // 1: the shapes the keep rule confirmed only (DESIGN.md 5 "Pixel layer").
      const bool pixel_shape = pixel_cache == 2 ||
                               (pixel_cache == 1 && f.ss == 0 && f.n <= sfrt::kInlineSpheres &&
                                sfrt::compact_eligible(recs.data(), f.n, f.ss));
      const bool pixel_layer = pixels && texels && pixel_shape && !sfrt::kDiagnosticBuild &&
                               d_pixel_status && sfrt::pixel_copy_fits(f);
      const sfrt::CacheSizes sizes{sfrt::ray_cache_bytes(tiles, rays), sfrt::tile_rec_bytes(tiles),
                                   sfrt::cull_rec_bytes(tiles),
                                   sfrt::cull_win_bytes(tiles, f.n > sfrt::kInlineSpheres),
                                   sfrt::hit_cache_bytes(tiles, rays),
                                   texels ? sfrt::texel_cache_bytes(tiles, rays) : 0,
                                   compact ? sfrt::compact_cache_bytes(tiles, rays) : 0,
                                   pixel_layer ? sfrt::pixel_cache_bytes(f.sub_w >> f.ss, f.sub_rows >> f.ss) : 0};
      // (the diagnostic builds exist to time the march: no hit cache)
      launch_caches = mine.begin(cull_key.ray, cull_key, sizes,
                                 cache_bytes_held() - mine.bytes_under_ray_budget(),
                                 hit_bytes_budgeted() - mine.bytes_under_hit_budget(),
                                 (long long)ray_cache_mb << 20,
                                 sfrt::kDiagnosticBuild ? 0 : hit_budget_bytes(), CacheDevice{s, f, recs},
                                 texels ? &tex_key : nullptr, compact, pixel_layer ? tex_generation : -1);
      if (launch_caches.pixel != sfrt::RayAction::kTrace) launch_caches.pixel_status = d_pixel_status + cur_chain;
      if (launch_caches.compact != sfrt::RayAction::kTrace) {
        launch_caches.bright_rep = d_bright_rep;
        launch_caches.bright_classes = sfrt::BrightClasses::get().classes();
      }
      // A reading launch marches nothing and takes no part in the tile order: nothing is linked.
      if (launch_caches.reading()) {
        sfrt::TileSchedPtrs{}.link(f);
        f.order_dilate = 0;
      }
    }
    return SFRT_OK;
  }

  static void make_cull_key(sfrt::CullKey& k, const sfrt::RayKey& ray, const sfrt::FrameRec& f,
                            const std::vector<sfrt::SphereRec>& recs) {
    k.ray = ray;
    for (int q = 0; q < 3; q++) k.cam[q] = sfrt::ray_key_bits(f.cam[q]);
    k.cull_margin = sfrt::ray_key_bits(f.cull_margin);
    k.first_l = sfrt::ray_key_bits(f.first_l);
    k.cull = f.cull;  // the option, cleared by prepare_frame for non-finite inputs
    k.set_records(recs.data(), f.n);
  }

  // k.cull is the launch's CullKey already (sched_begin); tex_off and tex_wh as prepare_records
  // wrote them.
  static void make_tex_key(sfrt::TexKey& k, const std::vector<sfrt::SphereRec>& recs, int n) {
    k.set_textures(recs.data(), n);
  }

  // The class table on the device, at world creation (128 KiB, off the render path): the entries
  // past the last class repeat it, so that every class a record's 15 bits can name is readable.
  // A failure is no error of the world: the compact layer is never filled.
  void upload_bright_rep() {
    if (!sfrt::BrightClasses::get().fits()) return;
    std::vector<uint32_t> rep = sfrt::BrightClasses::get().rep;
    rep.resize(sfrt::kCompactClassLimit, rep.back());
    void* p = nullptr;
    if (hipMalloc(&p, rep.size() * 4) != hipSuccess ||
        hipMemcpy(p, rep.data(), rep.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      if (p) (void)hipFree(p);
      return;
    }
    d_bright_rep = (uint32_t*)p;
  }

  static sfrt::RayKey make_ray_key(const sfrt::FrameRec& f, long long tile_key) {
    sfrt::RayKey k{};
    for (int q = 0; q < 3; q++) {
      k.fwd[q] = sfrt::ray_key_bits(f.fwd[q]);
      k.right[q] = sfrt::ray_key_bits(f.right[q]);
      k.up[q] = sfrt::ray_key_bits(f.up[q]);
    }
    k.h_start = sfrt::ray_key_bits(f.h_start); k.h_inc = sfrt::ray_key_bits(f.h_inc);
    k.v_start = sfrt::ray_key_bits(f.v_start); k.v_inc = sfrt::ray_key_bits(f.v_inc);
    k.xstart = f.xstart; k.xadd = f.xadd; k.ystart = f.ystart; k.yadd = f.yadd;
    k.sub_w = f.sub_w; k.sub_row0 = f.sub_row0; k.sub_rows = f.sub_rows;
    k.tile_key = tile_key;
    return k;
  }

  // A sum over the chains' caches.
  template <class Bytes>
  long long held(Bytes bytes) const {
    long long sum = 0;
    for (const sfrt::ChainCaches& c : caches) sum += bytes(c);
    return sum;
  }
  // SFRT_OPT_HIT_CACHE_MB in bytes: megabytes of 10^6 (sfrt.h says why), unlike the ray cache's MiB.
  long long hit_budget_bytes() const { return (long long)hit_cache_mb * 1000000ll; }
  // Everything SFRT_OPT_RAY_CACHE_MB limits (the directions and the cull caches); what
  // SFRT_OPT_HIT_CACHE_MB limits, and nothing else does.
  long long cache_bytes_held() const {
    return held([](const sfrt::ChainCaches& c) { return c.bytes_under_ray_budget(); });
  }
  long long hit_bytes_held() const {  // the hit records alone (sfrt_world_hit_cache_stats)
    return held([](const sfrt::ChainCaches& c) { return c.hit_bytes(); });
  }
  long long texel_bytes_held() const {
    return held([](const sfrt::ChainCaches& c) { return c.texel_bytes(); });
  }
  long long compact_bytes_held() const {
    return held([](const sfrt::ChainCaches& c) { return c.compact_bytes(); });
  }
  long long pixel_bytes_held() const {
    return held([](const sfrt::ChainCaches& c) { return c.pixel_bytes(); });
  }
  long long hit_bytes_budgeted() const {  // with the texel records: what the option limits
    return held([](const sfrt::ChainCaches& c) { return c.bytes_under_hit_budget(); });
  }

  // The device as a chain's caches see it (ChainCaches::begin): buffers freed and allocated in
  // the order of s, where the chain's launches run (sched.begin has waited for the device if
  // another stream ran the last one), and the fill kernels for f and recs queued on s.
  struct CacheDevice {
    hipStream_t s;
    const sfrt::FrameRec& f;
    const std::vector<sfrt::SphereRec>& recs;
    bool free(void* p) const {
      if (hipFreeAsync(p, s) == hipSuccess) return true;
      (void)hipGetLastError();
      return false;
    }
    void* alloc(long long n) const {
      void* p = nullptr;
      if (hipMallocAsync(&p, (size_t)n, s) == hipSuccess) return p;
      (void)hipGetLastError();  // no memory for it: not an error of the frame
      return nullptr;
    }
    bool fill_rays(float* dirs, sfrt::TileRec* tile_recs) const {
      return sfrt::launch_ray_fill(f, dirs, tile_recs, s) == 0;
    }
    bool fill_cull(const sfrt::TileRec* tile_recs, sfrt::CullRec* cull_recs, void* cull_wins) const {
      return sfrt::launch_cull_fill(f, recs.data(), tile_recs, cull_recs, cull_wins, s) == 0;
    }
  };

  // An option lowered below what the chains hold (hit_only: SFRT_OPT_HIT_CACHE_MB, the hit caches
  // go; else SFRT_OPT_RAY_CACHE_MB, every cache goes).  The chains' streams may be gone
  // (sfrt_sched.h), so the host waits for the device.
  // texel_only: SFRT_OPT_TEXEL_CACHE, that layer (and the compact one on it) alone;
  // compact_only: SFRT_OPT_COMPACT_TEXELS, that layer (and the pixel layer on it) alone;
  // pixel_only: SFRT_OPT_PIXEL_CACHE, that layer alone.
  int release_caches(bool hit_only, bool texel_only = false, bool compact_only = false,
                     bool pixel_only = false) {
    HIP_TRY(hipDeviceSynchronize());
    const auto free_now = [](void* p) { return hipFree(p) == hipSuccess; };
    for (sfrt::ChainCaches& c : caches) {
      if (pixel_only) c.release_pixel(free_now);
      else if (compact_only) c.release_compact(free_now);
      else if (texel_only) c.release_texel(free_now);
      else if (hit_only) c.release_hit(free_now);
      else c.release_all(free_now);
    }
    return SFRT_OK;
  }

  // After launch_trace for f returned (queued = false: it failed).
  int sched_end(const sfrt::FrameRec& f, hipStream_t s, bool queued) {
    sfrt::TileSchedPtrs p;
    p.tile_cost = f.tile_cost;
    sfrt::TileSched& sched = scheds.chain[cur_chain];
    sfrt::ChainCaches& mine = caches[cur_chain];
    if (queued && launch_caches.reading()) {
      // A launch that read the hit cache: the chain does not advance, and last_fill and the
      // chain's camera stay the last marching launch's (their classes are this frame's too: the
      // key is equal).
      sched.end_reading(s);
      mine.end(launch_caches, true, cache_stats);
      return SFRT_OK;
    }
    if (!queued && launch_caches.reading()) sched.reset();  // linked into nothing: end() would pass it by
    HIP_TRY(sched.end(p, s, queued));
    if (!queued) {
      // the failed launch of a chain -- an aux band's too -- leaves no cache to trust
      if (p.tile_cost || launch_caches.decided) mine.end(launch_caches, false, cache_stats);
      chain_cam[cur_chain].valid = false;
      if (last_fill.chain == cur_chain) last_fill.valid = false;
      return SFRT_E_HIP;
    }
    if (launch_caches.decided) mine.end(launch_caches, true, cache_stats);
    if (sched.committed) {
      chain_cam[cur_chain] = ChainCam{true, cam, f.sub_row0};
      // that launch wrote its classes into cost[k % 2] before end() advanced k
      last_fill = LastFill{true, f.sub_row0 >> f.ss, f.sub_rows >> f.ss, f.sub_w, sched.key_prev,
                           (int)((sched.k - 1) & 1), cur_chain, f.ss};
    } else {
      last_fill.valid = false;  // this fill recorded no classes (tile order off, probe)
    }
    return SFRT_OK;
  }

  // The last launch that recorded its per-tile march-step classes (sfrt_world_row_costs).
  struct LastFill {
    bool valid = false;
    int row0 = 0, rows = 0, width = 0;  // output rows; the grid's width (in samples when ss > 0)
    long long key = 0;  // trace_tile_key: pixels per lane, the tile grid and the factor
    int buf = 0;        // scheds.chain[chain].cost[buf]
    int chain = -1;
    int ss = 0;         // SFRT_OPT_SUPERSAMPLE (log2) of that fill: its tiles are of samples
  };
  LastFill last_fill;

  // The camera of the last launch that joined the tile-order chain: its costs are the
  // ones the next launch's sorter ranks.
  struct ChainCam {
    bool valid = false;
    sfrt_camera cam{};
    int sub_row0 = 0;
  };
  ChainCam chain_cam[sfrt::TileChains::kChains];  // per chain

  int read_status(hipStream_t s) {
    int st = 0;
    HIP_TRY(sfrt::read_status(d_status, s, &st));
    if (st & 1) return SFRT_E_MARCH_LIMIT;
    if (st & 2) return SFRT_E_TEXEL;
    return SFRT_OK;
  }
};

namespace {

// Representative march steps of a tile-order class (the inverse of sfrt_device.h
// tile_bucket: class 15 - c holds steps < 4 for c = 0, 2c + 2 .. 2c + 3 for c = 1..6,
// 16 + 4 (c - 7) .. + 3 for c = 7..10, then 32-39, 40-47, 48-63, 64-95, >= 96).
double class_steps(uint8_t cls) {
  const int c = 15 - (int)(cls & 15);
  if (c == 0) return 3.0;
  if (c <= 6) return 2.0 * c + 2.5;
  if (c <= 10) return 16.0 + 4.0 * (c - 7) + 1.5;
  static const double tail[5] = {35.5, 43.5, 55.5, 79.5, 128.0};
  return tail[c - 11];
}

// The shading tail costs about as much as four march steps per pixel (22% of
// the 4K frame, whose tiles march ~14 steps).
constexpr double kShadeSteps = 4.0;

}  // namespace

extern "C" {

int sfrt_world_row_costs(sfrt_world* w, float* costs, int capacity, int* row0, int* rows) {
  if (!w || !row0 || !rows || capacity < 0 || (capacity > 0 && !costs)) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *row0 = 0;
  *rows = 0;
  const auto& L = w->last_fill;
  if (!L.valid) return SFRT_E_INVALID;
  const int tile_w = (int)((L.key >> 56) & 0x7) * sfrt::kTile;
  const long long tiles_x = (L.key >> 28) & 0xfffffff, tiles_y = L.key & 0xfffffff;
  const sfrt::TileSched& sched = w->scheds.chain[L.chain];
  if (tile_w <= 0 || tiles_x * tiles_y > sched.cap) return SFRT_E_INVALID;
  // a fill at one factor is never read back as another: the key carries the factor
  if ((int)((L.key >> 59) & 3) != L.ss || L.ss != w->ss) return SFRT_E_INVALID;
  if (capacity < L.rows) return SFRT_E_INVALID;
  sfrt::DeviceGuard g(w->device);
  // the chain's last launch may still be running on a stream the caller has since destroyed
  // (its handle must not be used, sfrt_sched.h): a tuning call, it waits for the device
  if (sched.have_last) HIP_TRY(hipDeviceSynchronize());
  std::vector<uint8_t> cls((size_t)(tiles_x * tiles_y));
  HIP_TRY(hipMemcpy(cls.data(), sched.cost[L.buf], cls.size(), hipMemcpyDeviceToHost));
  for (long long ty = 0; ty < tiles_y; ty++) {
    double c = 0.0;
    for (long long tx = 0; tx < tiles_x; tx++) {
      const long long x0 = tx * tile_w;
      const long long px = std::min<long long>(tile_w, L.width - x0);
      c += (class_steps(cls[(size_t)(ty * tiles_x + tx)]) + kShadeSteps) * (double)px;
    }
    // Supersampled: the tile's 8 sample rows are 8 / S output rows, and an output row costs
    // its S sample rows (all in this tile row: S divides 8 and the band starts on a group).
    const int tile_rows = sfrt::kTile >> L.ss;
    for (int j = (int)ty * tile_rows; j < std::min(L.rows, (int)(ty + 1) * tile_rows); j++)
      costs[j] = (float)(c * (double)(1 << L.ss));
  }
  *row0 = L.row0;
  *rows = L.rows;
  return SFRT_OK;
}

int sfrt_world_create(int hip_device, sfrt_world** out) {
  if (!out) return SFRT_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || hip_device < 0 || hip_device >= count)
    return SFRT_E_HIP;
  sfrt_world* w = new sfrt_world();
  w->device = hip_device;
  w->tex_written.relay = &w->relay;
  for (sfrt::TableSlot& t : w->view_slots) t.relay = &w->relay;
  // Camera defaults (SphereWorld.h:10-21) and the constructor's conversion (:72-73).
  w->cam.fov_h = sfrt_deg_to_rad(75.0f);
  w->cam.fov_v = sfrt_deg_to_rad(47.0f);
  sfrt::DeviceGuard g(hip_device);
  if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&w->d_status, sizeof(int)) != hipSuccess ||
      hipMemset(w->d_status, 0, sizeof(int)) != hipSuccess) {
    delete w;
    return SFRT_E_HIP;
  }
  // (a failure is no error of the world: the pixel layer is never filled)
  if (hipMalloc(&w->d_pixel_status, sizeof(int) * sfrt::TileChains::kChains) != hipSuccess ||
      hipMemset(w->d_pixel_status, 0, sizeof(int) * sfrt::TileChains::kChains) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(w->d_pixel_status);
    w->d_pixel_status = nullptr;
  }
  w->upload_bright_rep();
  *out = w;
  return SFRT_OK;
}

void sfrt_world_destroy(sfrt_world* w) { delete w; }

int sfrt_world_set_size(sfrt_world* w, int width, int height) {
  if (!w || width <= 0 || height <= 0) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if (width != w->width || height != w->height) {
    // the last fill's rows and tile grid belong to the old frame (sfrt_world_row_costs)
    w->last_fill.valid = false;
    for (auto& c : w->chain_cam) c.valid = false;
  }
  w->width = width;
  w->height = height;
  return SFRT_OK;
}

int sfrt_world_get_size(const sfrt_world* w, int* width, int* height) {
  if (!w || !width || !height) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *width = w->width;
  *height = w->height;
  return SFRT_OK;
}

int sfrt_world_set_camera(sfrt_world* w, const sfrt_camera* cam) {
  if (!w || !cam || !camera_ok(*cam)) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  w->cam = *cam;
  return SFRT_OK;
}

int sfrt_world_get_camera(const sfrt_world* w, sfrt_camera* cam) {
  if (!w || !cam) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *cam = w->cam;
  return SFRT_OK;
}

int sfrt_world_load_texture(sfrt_world* w, int slot, const uint8_t* rgba, int tex_w, int tex_h) {
  if (!w || !rgba || slot < 0 || slot >= SFRT_TEXTURE_SLOTS || tex_w <= 0 || tex_h <= 0 ||
      tex_w > 0xffff || tex_h > 0xffff || (int64_t)tex_w * tex_h > (1 << 28))
    return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  const size_t bytes = (size_t)tex_w * tex_h * 4;
  w->tex_generation++;  // whatever becomes of this call: no cached pixel outlives it
  w->tex_host[slot].assign(rgba, rgba + bytes);
  w->tex_w[slot] = tex_w;
  w->tex_h[slot] = tex_h;
  bool a01 = true;
  for (size_t i = 3; i < bytes && a01; i += 4) a01 = rgba[i] == 0 || rgba[i] == 255;
  w->tex_alpha01[slot] = a01;
  int one = rgba[3];
  for (size_t i = 3; i < bytes && one >= 0; i += 4) one = rgba[i] == one ? one : -1;
  w->tex_alpha_one[slot] = one;
  // Rebuild the device atlas: textures[0] (SphereWorld.cpp:376-377) first, then
  // the extension slots.  Draws on any stream may still read the old atlas.
  size_t total = 0;
  for (int k = 0; k < SFRT_TEXTURE_SLOTS; k++) {
    w->tex_off[k] = (uint32_t)total;
    total += (size_t)w->tex_w[k] * w->tex_h[k];
  }
  if (total > 0xffffffffull) return SFRT_E_INVALID;
  sfrt::DeviceGuard g(w->device);
  // Stream-ordered (no device-wide wait): a new atlas (hipMalloc waits for no stream,
  // profiles/r6u_hip_alloc_calls.txt), uploaded on the world's stream from pinned staging.
  void* staged = nullptr;
  HIP_TRY(w->tex_stage.take(total * 4, &staged));
  for (int k = 0; k < SFRT_TEXTURE_SLOTS; k++)
    if (!w->tex_host[k].empty())
      std::memcpy((uint8_t*)staged + (size_t)w->tex_off[k] * 4, w->tex_host[k].data(),
                  w->tex_host[k].size());
  uint32_t* fresh = nullptr;
  HIP_TRY(hipMalloc(&fresh, total * 4));
  if (hipMemcpyAsync(fresh, staged, total * 4, hipMemcpyHostToDevice, w->stream) != hipSuccess ||
      w->tex_stage.copied(w->stream) != hipSuccess || w->tex_written.after_write(w->stream) != hipSuccess) {
    (void)hipStreamSynchronize(w->stream);
    (void)hipFree(fresh);
    return SFRT_E_HIP;
  }
  if (w->d_tex) {
    w->retired_tex.push_back(w->d_tex);
    w->retired_tex_bytes += w->d_tex_texels * 4;
  }
  w->d_tex = fresh;
  w->d_tex_texels = total;
  if (w->retired_tex_bytes > sfrt_world::kRetiredTexBytes) {  // a texture reloaded every frame
    HIP_TRY(hipDeviceSynchronize());
    for (void* p : w->retired_tex) (void)hipFree(p);
    w->retired_tex.clear();
    w->retired_tex_bytes = 0;
  }
  return SFRT_OK;
}

int sfrt_world_alpha_binary(const sfrt_world* w, int* binary) {
  if (!w || !binary) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  // Supersampled, a pixel's alpha is the rounded mean of S*S texel alphas: 0 or 255 for every
  // pixel only if all loaded texels share one of the two (the mean of equal values is the value).
  bool any = false, all = true;
  int one = -2;  // the alpha shared so far (-2: none seen, -1: they differ)
  for (int k = 0; k < SFRT_TEXTURE_SLOTS; k++) {
    if (w->tex_host[k].empty()) continue;
    any = true;
    all = all && w->tex_alpha01[k];
    one = one == -2 || one == w->tex_alpha_one[k] ? w->tex_alpha_one[k] : -1;
  }
  *binary = any && all && (w->ss == 0 || one >= 0) ? 1 : 0;
  return SFRT_OK;
}

int sfrt_world_add_sphere(sfrt_world* w, float x, float y, float z, float radius) {
  const sfrt_sphere add{x, y, z, radius};
  if (!w || !sphere_ok(add)) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  std::vector<sfrt_sphere>& s = w->spheres;
  std::vector<int32_t>& st = w->sphere_tex;
  s.push_back(add);
  st.push_back(0);
  // SphereWorld.cpp:180-188: drop every sphere contained in another one.
  for (int i = 0; i < (int)s.size(); i++) {
    for (int j = 0; j < (int)s.size(); j++) {
      if (i != j && vlength(vsub(center(s[i]), center(s[j]))) + s[i].radius <= s[j].radius) {
        s.erase(s.begin() + i);
        st.erase(st.begin() + i);
        i--;
        break;
      }
    }
  }
  permute(st, sort_spheres(s, {w->cam.pos[0], w->cam.pos[1], w->cam.pos[2]}));
  if ((int)s.size() > SFRT_MAX_SPHERES) return SFRT_E_TOO_MANY;
  return SFRT_OK;
}

int sfrt_world_set_spheres(sfrt_world* w, const sfrt_sphere* spheres, int count) {
  if (!w || count < 0 || (count > 0 && !spheres)) return SFRT_E_INVALID;
  if (count > SFRT_MAX_SPHERES) return SFRT_E_TOO_MANY;
  for (int i = 0; i < count; i++)
    if (!sphere_ok(spheres[i])) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  w->spheres.assign(spheres, spheres + count);
  w->sphere_tex.assign((size_t)count, 0);
  return SFRT_OK;
}

int sfrt_world_set_sphere_textures(sfrt_world* w, const int32_t* slots, int count) {
  if (!w || count < 0 || (count > 0 && !slots)) return SFRT_E_INVALID;
  for (int i = 0; i < count; i++)
    if (slots[i] < 0 || slots[i] >= SFRT_TEXTURE_SLOTS) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if ((size_t)count != w->spheres.size()) return SFRT_E_INVALID;
  w->sphere_tex.assign(slots, slots + count);
  return SFRT_OK;
}

int sfrt_world_get_sphere_textures(sfrt_world* w, int32_t* out, int capacity, int* count) {
  if (!w || !count) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *count = (int)w->sphere_tex.size();
  if (out) {
    const int n = capacity < *count ? capacity : *count;
    std::memcpy(out, w->sphere_tex.data(), sizeof(int32_t) * (size_t)(n > 0 ? n : 0));
  }
  return SFRT_OK;
}

int sfrt_world_get_spheres(const sfrt_world* w, sfrt_sphere* out, int capacity, int* count) {
  if (!w || !count) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *count = (int)w->spheres.size();
  if (out) {
    const int n = capacity < *count ? capacity : *count;
    std::memcpy(out, w->spheres.data(), sizeof(sfrt_sphere) * (size_t)(n > 0 ? n : 0));
  }
  return SFRT_OK;
}

int sfrt_world_update_spheres(sfrt_world* w) {
  if (!w) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  permute(w->sphere_tex, sort_spheres(w->spheres, {w->cam.pos[0], w->cam.pos[1], w->cam.pos[2]}));
  return SFRT_OK;
}

int sfrt_world_set_option(sfrt_world* w, int option, int value) {
  if (!w) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if (option == SFRT_OPT_CULL) {
    w->cull = value ? 1 : 0;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_RAYS_PER_LANE) {
    if (value < 0 || value > 4) return SFRT_E_INVALID;
    w->rays = value;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_TILE_ORDER) {
    w->tile_order_on = value == 2 ? 2 : value ? 1 : 0;  // 2: timing probe (see sched_begin)
    return SFRT_OK;
  }
  if (option == SFRT_OPT_SUPERSAMPLE) {
    if (value != 1 && value != 2 && value != 4) return SFRT_E_INVALID;
    const int ss = value == 4 ? 2 : value == 2 ? 1 : 0;
    if (ss != w->ss) {
      // the last fill's tiles and the chains' recorded costs belong to the old sample grid
      w->last_fill.valid = false;
      for (auto& c : w->chain_cam) c.valid = false;
    }
    w->ss = ss;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_RAY_CACHE_MB) {
    if (value < 0) return SFRT_E_INVALID;
    // (0 also frees tile records left without directions by a fill that found no memory)
    if (((long long)value << 20) < w->cache_bytes_held() ||
        (value == 0 && w->held([](const sfrt::ChainCaches& c) { return c.tile_rec_bytes(); }) > 0)) {
      sfrt::DeviceGuard g(w->device);
      const int rc = w->release_caches(false);
      if (rc) return rc;
    }
    if (value == 0)
      for (sfrt::ChainCaches& c : w->caches) c.invalidate();
    w->ray_cache_mb = value;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_HIT_CACHE_MB) {
    if (value < 0) return SFRT_E_INVALID;
    if ((long long)value * 1000000ll < w->hit_bytes_budgeted()) {
      sfrt::DeviceGuard g(w->device);
      const int rc = w->release_caches(true);
      if (rc) return rc;
    }
    if (value == 0)
      for (sfrt::ChainCaches& c : w->caches) c.invalidate_hit();
    w->hit_cache_mb = value;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_TEXEL_CACHE) {
    if (value < 0) return SFRT_E_INVALID;
    if (value == 0) {
      if (w->texel_bytes_held() > 0) {
        sfrt::DeviceGuard g(w->device);
        const int rc = w->release_caches(false, true);
        if (rc) return rc;
      }
      for (sfrt::ChainCaches& c : w->caches) c.invalidate_texel();
    }
    w->texel_cache = value ? 1 : 0;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_COMPACT_TEXELS) {
    if (value < 0 || value > 2) return SFRT_E_INVALID;
    if (value < w->compact_texels) {  // (lowered: records of a shape no longer served would stay held)
      if (w->compact_bytes_held() > 0) {
        sfrt::DeviceGuard g(w->device);
        const int rc = w->release_caches(false, false, true);
        if (rc) return rc;
      }
      for (sfrt::ChainCaches& c : w->caches) c.invalidate_compact();
    }
    w->compact_texels = value;
    return SFRT_OK;
  }
  if (option == SFRT_OPT_PIXEL_CACHE) {
    if (value < 0 || value > 2) return SFRT_E_INVALID;
    if (value < w->pixel_cache) {  // (lowered: pixels of a shape no longer served would stay held)
      if (w->pixel_bytes_held() > 0) {
        sfrt::DeviceGuard g(w->device);
        const int rc = w->release_caches(false, false, false, true);
        if (rc) return rc;
      }
      for (sfrt::ChainCaches& c : w->caches) c.invalidate_pixel();
    }
    w->pixel_cache = value;
    return SFRT_OK;
  }
  return SFRT_E_INVALID;
}

int sfrt_world_ray_cache_stats(const sfrt_world* w, int64_t* cached_frames, int64_t* fills,
                               int64_t* bytes) {
  if (!w || !cached_frames || !fills || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *cached_frames = w->cache_stats.ray_cached_frames;
  *fills = w->cache_stats.ray_fills;
  *bytes = w->held([](const sfrt::ChainCaches& c) { return c.dirs.bytes; });
  return SFRT_OK;
}

int sfrt_world_cull_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits, int64_t* bytes) {
  if (!w || !fills || !hits || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *fills = w->cache_stats.cull_fills;
  *hits = w->cache_stats.cull_hits;
  *bytes = w->held([](const sfrt::ChainCaches& c) { return c.cull_bytes(); });
  return SFRT_OK;
}

int sfrt_world_hit_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits, int64_t* bytes) {
  if (!w || !fills || !hits || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *fills = w->cache_stats.hit_fills;
  *hits = w->cache_stats.hit_hits;
  *bytes = w->hit_bytes_held();
  return SFRT_OK;
}

int sfrt_world_texel_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits, int64_t* bytes) {
  if (!w || !fills || !hits || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *fills = w->cache_stats.texel_fills;
  *hits = w->cache_stats.texel_hits;
  *bytes = w->texel_bytes_held();
  return SFRT_OK;
}

int sfrt_world_compact_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits, int64_t* bytes) {
  if (!w || !fills || !hits || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *fills = w->cache_stats.compact_fills;
  *hits = w->cache_stats.compact_hits;
  *bytes = w->compact_bytes_held();
  return SFRT_OK;
}

int sfrt_world_pixel_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits, int64_t* bytes) {
  if (!w || !fills || !hits || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *fills = w->cache_stats.pixel_fills;
  *hits = w->cache_stats.pixel_hits;
  *bytes = w->pixel_bytes_held();
  return SFRT_OK;
}

int sfrt_world_tile_record_bytes(const sfrt_world* w, int64_t* bytes) {
  if (!w || !bytes) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  *bytes = w->held([](const sfrt::ChainCaches& c) { return c.tile_rec_bytes(); });
  return SFRT_OK;
}

int sfrt_world_get_option(const sfrt_world* w, int option, int* value) {
  if (!w || !value) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  switch (option) {
    case SFRT_OPT_CULL: *value = w->cull; return SFRT_OK;
    case SFRT_OPT_RAYS_PER_LANE: *value = w->rays; return SFRT_OK;
    case SFRT_OPT_TILE_ORDER: *value = w->tile_order_on; return SFRT_OK;
    case SFRT_OPT_SUPERSAMPLE: *value = 1 << w->ss; return SFRT_OK;
    case SFRT_OPT_RAY_CACHE_MB: *value = w->ray_cache_mb; return SFRT_OK;
    case SFRT_OPT_HIT_CACHE_MB: *value = w->hit_cache_mb; return SFRT_OK;
    case SFRT_OPT_TEXEL_CACHE: *value = w->texel_cache; return SFRT_OK;
    case SFRT_OPT_COMPACT_TEXELS: *value = w->compact_texels; return SFRT_OK;
    case SFRT_OPT_PIXEL_CACHE: *value = w->pixel_cache; return SFRT_OK;
    default: return SFRT_E_INVALID;
  }
}

// sfrt_world_update_image and sfrt_world_update_image_aux (planes: depth, sphere, steps as
// host planes of width*height elements, any null; nullptr for the plain call).
static int update_image_body(sfrt_world* w, uint8_t* pixels, void* const* planes, int ystart,
                             int yadd, int xstart, int xadd) {
  if (!w || !pixels || ystart < 0 || xstart < 0 || yadd <= 0 || xadd <= 0) return SFRT_E_INVALID;
  if (planes && !planes[0] && !planes[1] && !planes[2]) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  int rc = w->validate();
  if (rc) return rc;
  // SphereWorld.cpp:94,97: i = xstart, xstart + xadd, ... < width (same for j).
  const int sub_w = xstart < w->width ? (w->width - xstart + xadd - 1) / xadd : 0;
  const int sub_h = ystart < w->height ? (w->height - ystart + yadd - 1) / yadd : 0;
  if (sub_w == 0 || sub_h == 0) return SFRT_OK;
  sfrt::DeviceGuard g(w->device);
  const size_t px = (size_t)sub_w * sub_h;
  // Growth waits for no other stream (sfrt_host.h): the device frame in the order of the world's
  // stream, behind the last update_image (which waited for its own copy).
  HIP_TRY(w->d_frame.reserve(px * 4, w->stream));
  HIP_TRY(w->h_stage.reserve(px * 4));
  for (int q = 0; planes && q < 3; q++)
    if (planes[q]) {
      HIP_TRY(w->d_aux[q].reserve(px * 4, w->stream));
      HIP_TRY(w->h_aux[q].reserve(px * 4));
    }
  sfrt::FrameRec f;
  std::vector<sfrt::SphereRec> recs;
  // Supersampled (S = 1 << ss): S x S samples per addressed pixel, start and strides in samples
  // (sfrt_trace.h FrameRec); d_frame and the scatter below stay in output pixels.
  // A stride that addresses one pixel only is never applied (and may not fit once scaled); the
  // others are below width / height, which validate() bounds.
  const int ss = w->ss;
  w->prepare(f, recs, ss);
  f.xstart = xstart << ss; f.xadd = (ss && sub_w == 1 ? 1 : xadd) << ss;
  f.ystart = ystart << ss; f.yadd = (ss && sub_h == 1 ? 1 : yadd) << ss;
  f.sub_w = sub_w << ss;
  f.sub_row0 = 0;
  f.sub_rows = sub_h << ss;
  f.tiles_x = (f.sub_w + sfrt::kTile - 1) / sfrt::kTile;
  f.out = w->d_frame.ptr<uint32_t>();
  f.out_pitch = sub_w;
  sfrt::AuxArgs aux{};
  if (planes) {  // compact planes beside the compact frame
    aux.depth = planes[0] ? w->d_aux[0].ptr<float>() : nullptr;
    aux.sphere = planes[1] ? w->d_aux[1].ptr<int32_t>() : nullptr;
    aux.steps = planes[2] ? w->d_aux[2].ptr<int32_t>() : nullptr;
    aux.depth_pitch = aux.sphere_pitch = aux.steps_pitch = sub_w;
  }
  if ((rc = w->launchable(f))) return rc;
  rc = w->stage_spheres(f, recs, w->stream, false);
  if (rc) return rc;
  if (sfrt::launch_trace(f, recs.data(), w->stream, nullptr, w->ring_event(), nullptr,
                         planes ? &aux : nullptr))
    return SFRT_E_HIP;
  if ((rc = w->launched_with())) return rc;
  HIP_TRY(hipMemcpyAsync(w->h_stage.ptr(), w->d_frame.ptr(), px * 4, hipMemcpyDeviceToHost, w->stream));
  for (int q = 0; planes && q < 3; q++)
    if (planes[q])
      HIP_TRY(hipMemcpyAsync(w->h_aux[q].ptr(), w->d_aux[q].ptr(), px * 4, hipMemcpyDeviceToHost,
                             w->stream));
  rc = w->read_status(w->stream);
  // the planes do not depend on the texel: a frame whose status is SFRT_E_TEXEL has them defined
  if (rc && !(planes && rc == SFRT_E_TEXEL)) return rc;
  // Scatter the subset into the caller's frame: only addressed pixels are written.
  const auto scatter = [&](const sfrt::PinnedBuf& stage, void* dst) {
    sfrt::scatter_subset(stage.ptr<uint32_t>(), (uint8_t*)dst, (size_t)w->width, sub_w, sub_h,
                         xstart, xadd, ystart, yadd);
  };
  if (!rc) scatter(w->h_stage, pixels);
  for (int q = 0; planes && q < 3; q++)
    if (planes[q]) scatter(w->h_aux[q], planes[q]);
  return rc;
}

int sfrt_world_update_image(sfrt_world* w, uint8_t* pixels, int ystart, int yadd, int xstart,
                            int xadd) {
  return update_image_body(w, pixels, nullptr, ystart, yadd, xstart, xadd);
}

int sfrt_world_update_image_aux(sfrt_world* w, uint8_t* pixels, float* depth, int32_t* sphere,
                                int32_t* steps, int ystart, int yadd, int xstart, int xadd) {
  void* const planes[3] = {depth, sphere, steps};
  return update_image_body(w, pixels, planes, ystart, yadd, xstart, xadd);
}

// sfrt_world_render_band and sfrt_world_render_band_aux (aux: nullptr for the plain call).
static int render_band_body(sfrt_world* w, void* dev_pixels, int64_t pitch_bytes,
                            const sfrt_aux_planes* aux, bool with_aux, int row0, int rows,
                            void* hip_stream) {
  if (!w || !dev_pixels || row0 < 0 || rows < 0 || pitch_bytes % 4 != 0) return SFRT_E_INVALID;
  if (with_aux && (!aux || (!aux->depth && !aux->sphere && !aux->steps))) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  int rc = w->validate();
  if (rc) return rc;
  if (pitch_bytes < (int64_t)w->width * 4 || row0 + rows > w->height) return SFRT_E_INVALID;
  sfrt::AuxArgs a{};
  if (with_aux &&
      (!sfrt::aux_plane(aux->depth, aux->depth_pitch_bytes, w->width, a.depth, a.depth_pitch) ||
       !sfrt::aux_plane(aux->sphere, aux->sphere_pitch_bytes, w->width, a.sphere, a.sphere_pitch) ||
       !sfrt::aux_plane(aux->steps, aux->steps_pitch_bytes, w->width, a.steps, a.steps_pitch)))
    return SFRT_E_INVALID;
  if (rows == 0) {
    w->last_fill.valid = false;  // the last fill covered no rows (sfrt_world_row_costs)
    return SFRT_OK;
  }
  sfrt::DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)hip_stream;  // HIP convention: NULL = the null stream
  sfrt::FrameRec f;
  std::vector<sfrt::SphereRec> recs;
  const int ss = w->ss;  // supersampled: the band's S*rows sample rows of the S*width sample frame
  w->prepare(f, recs, ss);
  f.xstart = 0; f.xadd = 1 << ss; f.ystart = 0; f.yadd = 1 << ss;
  f.sub_w = w->width << ss;
  f.sub_row0 = row0 << ss;
  f.sub_rows = rows << ss;
  f.tiles_x = (f.sub_w + sfrt::kTile - 1) / sfrt::kTile;
  f.out = (uint32_t*)dev_pixels;
  f.out_pitch = pitch_bytes / 4;
  if ((rc = w->launchable(f))) return rc;
  rc = w->stage_spheres(f, recs, s, false);
  if (rc) return rc;
  // after the last texture upload (queued on w->stream, where the other launches run)
  HIP_TRY(w->tex_written.before_read(s));
  if ((rc = w->sched_begin(f, recs, s, with_aux, !with_aux))) return rc;
  if ((rc = w->sched_end(f, s, sfrt::launch_trace(f, recs.data(), s, nullptr, w->ring_event(),
                                                  &w->launch_caches, with_aux ? &a : nullptr) == 0)))
    return rc;
  if ((rc = w->launched_with())) return rc;
  return SFRT_OK;
}

int sfrt_world_render_band(sfrt_world* w, void* dev_pixels, int64_t pitch_bytes, int row0,
                           int rows, void* hip_stream) {
  return render_band_body(w, dev_pixels, pitch_bytes, nullptr, false, row0, rows, hip_stream);
}

int sfrt_world_render_band_aux(sfrt_world* w, void* dev_pixels, int64_t pitch_bytes,
                               const sfrt_aux_planes* aux, int row0, int rows, void* hip_stream) {
  return render_band_body(w, dev_pixels, pitch_bytes, aux, true, row0, rows, hip_stream);
}

// sfrt_world_render_subset and sfrt_world_render_subset_aux (with_aux false for the plain call):
// update_image's subset walk and kernel table, stored in place in the caller's whole device frame
// (the placing kernels, sfrt_trace.h launch_trace) on the caller's stream.  Like update_image's own
// launch it is row-major and outside the tile-order chain: no sched_begin / sched_end, so the ray
// cache, the tile records and the last fill (sfrt_world_row_costs) are left as they are.
static int render_subset_body(sfrt_world* w, void* dev_frame, int64_t pitch_bytes,
                              const sfrt_aux_planes* aux, bool with_aux, int ystart, int yadd,
                              int xstart, int xadd, void* hip_stream) {
  if (!w || !dev_frame || ystart < 0 || xstart < 0 || yadd <= 0 || xadd <= 0 || pitch_bytes % 4 != 0)
    return SFRT_E_INVALID;
  if (with_aux && (!aux || (!aux->depth && !aux->sphere && !aux->steps))) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  int rc = w->validate();
  if (rc) return rc;
  if (pitch_bytes < (int64_t)w->width * 4) return SFRT_E_INVALID;
  sfrt::AuxArgs a{};
  if (with_aux &&
      (!sfrt::aux_plane(aux->depth, aux->depth_pitch_bytes, w->width, a.depth, a.depth_pitch) ||
       !sfrt::aux_plane(aux->sphere, aux->sphere_pitch_bytes, w->width, a.sphere, a.sphere_pitch) ||
       !sfrt::aux_plane(aux->steps, aux->steps_pitch_bytes, w->width, a.steps, a.steps_pitch)))
    return SFRT_E_INVALID;
  // SphereWorld.cpp:94,97: i = xstart, xstart + xadd, ... < width (same for j); 64-bit: a
  // stride near INT_MAX is a valid one-pixel subset
  const int sub_w = xstart < w->width ? (int)(((long long)w->width - xstart + xadd - 1) / xadd) : 0;
  const int sub_h = ystart < w->height ? (int)(((long long)w->height - ystart + yadd - 1) / yadd) : 0;
  if (sub_w == 0 || sub_h == 0) return SFRT_OK;
  sfrt::DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)hip_stream;  // HIP convention: NULL = the null stream
  sfrt::FrameRec f;
  std::vector<sfrt::SphereRec> recs;
  // the subset as update_image_body takes it (supersampled: in samples, a stride that addresses
  // one pixel only not scaled)
  const int ss = w->ss;
  w->prepare(f, recs, ss);
  f.xstart = xstart << ss; f.xadd = (ss && sub_w == 1 ? 1 : xadd) << ss;
  f.ystart = ystart << ss; f.yadd = (ss && sub_h == 1 ? 1 : yadd) << ss;
  f.sub_w = sub_w << ss;
  f.sub_row0 = 0;
  f.sub_rows = sub_h << ss;
  f.tiles_x = (f.sub_w + sfrt::kTile - 1) / sfrt::kTile;
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
    if (a.sphere) a.sphere += (long long)ystart * a.sphere_pitch + xstart;
    if (a.steps) a.steps += (long long)ystart * a.steps_pitch + xstart;
    a.depth_pitch *= row_mul; a.sphere_pitch *= row_mul; a.steps_pitch *= row_mul;
  }
  if ((rc = w->launchable(f))) return rc;
  rc = w->stage_spheres(f, recs, s, false);
  if (rc) return rc;
  // after the last texture upload (queued on w->stream, where the other launches run)
  HIP_TRY(w->tex_written.before_read(s));
  if (sfrt::launch_trace(f, recs.data(), s, nullptr, w->ring_event(), nullptr,
                         with_aux ? &a : nullptr, col_stride))
    return SFRT_E_HIP;
  return w->launched_with();
}

int sfrt_world_render_subset(sfrt_world* w, void* dev_frame, int64_t pitch_bytes, int ystart,
                             int yadd, int xstart, int xadd, void* hip_stream) {
  return render_subset_body(w, dev_frame, pitch_bytes, nullptr, false, ystart, yadd, xstart, xadd,
                            hip_stream);
}

int sfrt_world_render_subset_aux(sfrt_world* w, void* dev_frame, int64_t pitch_bytes,
                                 const sfrt_aux_planes* aux, int ystart, int yadd, int xstart,
                                 int xadd, void* hip_stream) {
  return render_subset_body(w, dev_frame, pitch_bytes, aux, true, ystart, yadd, xstart, xadd,
                            hip_stream);
}

// sfrt_world_render_views and sfrt_world_render_views_aux (with_aux false for the plain call): view
// k is the whole frame that set_camera(views[k].cam) [+ update_spheres] + render_band[_aux] would
// write, all views in one launch of the view kernels (sfrt_trace.h launch_trace_views).  Each view's
// record is prepare_frame's for its camera -- on a sorted copy of the spheres with SORT -- with the
// frame geometry of render_band_body; the records and the sphere tables (one shared table, or one
// per view with SORT, each at least kInlineSpheres records long) go to the device as one block of
// a table slot.  Nothing of the world is written: not the camera, the spheres or their slots, and,
// the launch being row-major and outside the tile-order chains as render_subset's, neither the ray
// cache, the tile records nor the last fill.
static int render_views_body(sfrt_world* w, const sfrt_view* views, const sfrt_aux_planes* planes,
                             bool with_aux, int count, int64_t pitch_bytes, int flags,
                             void* hip_stream) {
  if (!w || !views || count < 0 || count > SFRT_MAX_VIEWS || (flags & ~SFRT_VIEWS_SORT) != 0 ||
      pitch_bytes % 4 != 0 || (with_aux && !planes))
    return SFRT_E_INVALID;
  for (int k = 0; k < count; k++) {
    if (!views[k].dev_pixels || !sfrt::aligned4({views[k].dev_pixels}) || !camera_ok(views[k].cam))
      return SFRT_E_INVALID;
    if (with_aux && !planes[k].depth && !planes[k].sphere && !planes[k].steps) return SFRT_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  if (count == 0) return SFRT_OK;
  int rc = w->validate();
  if (rc) return rc;
  if (pitch_bytes < (int64_t)w->width * 4) return SFRT_E_INVALID;
  std::vector<sfrt::AuxArgs> aux(with_aux ? (size_t)count : 0);
  for (size_t k = 0; k < aux.size(); k++) {
    const sfrt_aux_planes& p = planes[k];
    sfrt::AuxArgs& a = aux[k];
    if (!sfrt::aux_plane(p.depth, p.depth_pitch_bytes, w->width, a.depth, a.depth_pitch) ||
        !sfrt::aux_plane(p.sphere, p.sphere_pitch_bytes, w->width, a.sphere, a.sphere_pitch) ||
        !sfrt::aux_plane(p.steps, p.steps_pitch_bytes, w->width, a.steps, a.steps_pitch))
      return SFRT_E_INVALID;
  }
  // The frame geometry of render_band_body for rows [0, height), the same for every view, and
  // the grid it gives: refused before anything is queued if the runtime cannot take it
  // (work-items per grid dimension are 32 bits, workgroups in all at most 2^31 - 1).
  const int ss = w->ss;
  const int n = (int)w->spheres.size();
  sfrt::FrameRec geo;
  std::memset(&geo, 0, sizeof geo);
  geo.n = n;
  geo.rays = w->rays;
  geo.ss = ss;
  geo.xstart = 0; geo.xadd = 1 << ss; geo.ystart = 0; geo.yadd = 1 << ss;
  geo.sub_w = w->width << ss;
  geo.sub_row0 = 0;
  geo.sub_rows = w->height << ss;
  long long tiles = 0;
  sfrt::trace_views_grid(geo, &geo.tiles_x, &tiles);
  if (tiles <= 0 || tiles * 64 > 0xffffffffLL || tiles * count > 0x7fffffffLL) return SFRT_E_INVALID;
  sfrt::DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)hip_stream;  // HIP convention: NULL = the null stream
  const bool sort = (flags & SFRT_VIEWS_SORT) != 0;
  std::vector<sfrt::SphereRec> recs;
  w->prepare_records(recs, w->spheres, w->sphere_tex);
  // The block: the view records, then the sphere tables (32-byte records, 32-byte aligned).
  const size_t table_recs = (size_t)std::max(n, sfrt::kInlineSpheres);
  const size_t table_bytes = table_recs * sizeof(sfrt::SphereRec);
  const size_t tables_at = ((size_t)count * sizeof(sfrt::ViewRec) + 31) / 32 * 32;
  const size_t bytes = tables_at + (sort ? (size_t)count : 1) * table_bytes;
  sfrt::TableSlot& t = w->view_slots[w->next_view_slot];
  w->next_view_slot = (w->next_view_slot + 1) % sfrt_world::kViewSlots;
  HIP_TRY(t.reclaim());
  HIP_TRY(t.grow(bytes, s));
  uint8_t* const h = t.h.ptr<uint8_t>();
  uint8_t* const d = t.d.ptr<uint8_t>();
  std::memset(h + tables_at, 0, bytes - tables_at);  // the records past n: readable, never used
  if (!sort) std::memcpy(h + tables_at, recs.data(), sizeof(sfrt::SphereRec) * (size_t)n);
  std::vector<sfrt_sphere> sorted;
  for (int k = 0; k < count; k++) {
    const sfrt_camera& cam = views[k].cam;
    const size_t table_at = tables_at + (sort ? (size_t)k * table_bytes : 0);
    if (sort) {  // from the world's order, its records and their texture slots moved alike
      sorted = w->spheres;
      const std::vector<size_t> order = sort_spheres(sorted, {cam.pos[0], cam.pos[1], cam.pos[2]});
      sfrt::SphereRec* const dst = (sfrt::SphereRec*)(h + table_at);
      for (size_t i = 0; i < order.size(); i++) dst[i] = recs[order[i]];
    }
    sfrt::ViewRec v;
    std::memset(&v, 0, sizeof v);
    w->prepare_frame(v.f, cam, sort ? sorted : w->spheres, ss);
    v.f.xstart = geo.xstart; v.f.xadd = geo.xadd; v.f.ystart = geo.ystart; v.f.yadd = geo.yadd;
    v.f.sub_w = geo.sub_w;
    v.f.sub_row0 = geo.sub_row0;
    v.f.sub_rows = geo.sub_rows;
    v.f.tiles_x = geo.tiles_x;
    v.f.out = (uint32_t*)views[k].dev_pixels;
    v.f.out_pitch = pitch_bytes / 4;
    v.f.spheres = (const sfrt::SphereRec*)(d + table_at);
    if (with_aux) v.a = aux[(size_t)k];
    std::memcpy(h + (size_t)k * sizeof(sfrt::ViewRec), &v, sizeof v);
    if (k == 0) geo = v.f;  // the launch's own copy: any view's record names the kernel
  }
  HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  // after the last texture upload (queued on w->stream, where the other launches run)
  if (w->tex_written.before_read(s) != hipSuccess ||
      sfrt::launch_trace_views(geo, (const sfrt::ViewRec*)d, count, with_aux, s, t.launch_event())) {
    (void)t.staged(s);  // the copy is queued: the slot stays busy until it has run
    return SFRT_E_HIP;
  }
  HIP_TRY(t.launched_with(s));
  return SFRT_OK;
}

int sfrt_world_render_views(sfrt_world* w, const sfrt_view* views, int count, int64_t pitch_bytes,
                            int flags, void* hip_stream) {
  return render_views_body(w, views, nullptr, false, count, pitch_bytes, flags, hip_stream);
}

int sfrt_world_render_views_aux(sfrt_world* w, const sfrt_view* views, const sfrt_aux_planes* planes,
                                int count, int64_t pitch_bytes, int flags, void* hip_stream) {
  return render_views_body(w, views, planes, true, count, pitch_bytes, flags, hip_stream);
}

// sfrt_world_cast_rays_device and, for the host call's staged copies, sfrt_world_cast_rays:
// one launch of the ray-batch kernels on s with the world's mutex held.  The launch takes the
// frame fill's immutable snapshot (records in the kernel arguments, or a ring slot with its
// event) and nothing else of the world's: no tile-order chain, no ray cache, no last fill.
static int cast_rays_launch(sfrt_world* w, const float* dev_dirs, const float* dev_origins,
                            int64_t count, const sfrt_ray_hits& out, hipStream_t s) {
  sfrt::FrameRec f;
  std::vector<sfrt::SphereRec> recs;
  w->prepare(f, recs);
  int rc = w->stage_spheres(f, recs, s, false);
  if (rc) return rc;
  // after the last texture upload (queued on w->stream)
  if (out.rgba) HIP_TRY(w->tex_written.before_read(s));
  sfrt::RayArgs a{};
  a.dirs = dev_dirs;
  a.origins = dev_origins;
  a.count = count;
  a.pos = out.pos;
  a.depth = out.depth;
  a.sphere = out.sphere;
  a.steps = out.steps;
  a.rgba = (uint32_t*)out.rgba;
  if (sfrt::launch_cast_rays(f, recs.data(), a, s, w->ring_event())) return SFRT_E_HIP;
  return w->launched_with();
}

// What a batch needs of the world (mutex held); the argument checks: sfrt_host.h ray_hits_args.
static int cast_rays_world(const sfrt_world* w, bool rgba) {
  if (w->spheres.empty()) return SFRT_E_EMPTY;
  if ((int)w->spheres.size() > SFRT_MAX_SPHERES) return SFRT_E_TOO_MANY;
  if (!rgba) return SFRT_OK;  // pos, depth, sphere and steps need no texture
  if (w->tex_host[0].empty() || !w->d_tex) return SFRT_E_NO_TEXTURE;
  for (int32_t k : w->sphere_tex)
    if (w->tex_host[k].empty()) return SFRT_E_NO_TEXTURE;
  return SFRT_OK;
}

int sfrt_world_cast_rays_device(sfrt_world* w, const float* dev_dirs, const float* dev_origins,
                                int64_t count, const sfrt_ray_hits* dev_out, void* hip_stream) {
  int rc = sfrt::ray_hits_args(w, dev_dirs, dev_origins, count, dev_out);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(w->mu);
  if (count == 0) return SFRT_OK;
  if ((rc = cast_rays_world(w, dev_out->rgba != nullptr))) return rc;
  sfrt::DeviceGuard g(w->device);
  return cast_rays_launch(w, dev_dirs, dev_origins, count, *dev_out, (hipStream_t)hip_stream);
}

int sfrt_world_cast_rays(sfrt_world* w, const float* dirs, const float* origins, int64_t count,
                         const sfrt_ray_hits* out) {
  int rc = sfrt::ray_hits_args(w, dirs, origins, count, out);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(w->mu);
  if (count == 0) return SFRT_OK;
  if ((rc = cast_rays_world(w, out->rgba != nullptr))) return rc;
  sfrt::DeviceGuard g(w->device);
  const sfrt::BatchLayout l((size_t)count, {{dirs, 12}, {origins, 12}},
                            {{out->pos, 12}, {out->depth, 4}, {out->sphere, 4}, {out->steps, 4},
                             {out->rgba, 4}});
  HIP_TRY(w->ray_stage.upload(l, w->stream));
  void* const d = w->ray_stage.d.ptr();
  const sfrt_ray_hits dev{l.out_at<float>(d, 0), l.out_at<float>(d, 1), l.out_at<int32_t>(d, 2),
                          l.out_at<int32_t>(d, 3), l.out_at<uint8_t>(d, 4)};
  if ((rc = cast_rays_launch(w, l.in_at<float>(d, 0), l.in_at<float>(d, 1), count, dev, w->stream)))
    return rc;
  HIP_TRY(w->ray_stage.download(l, w->stream));
  rc = w->read_status(w->stream);
  // pos, depth, sphere and steps do not depend on the texel: all but rgba (output 4) are written
  if (rc && rc != SFRT_E_TEXEL) return rc;
  l.copy_outputs(w->ray_stage.h.ptr(), rc ? 1u << 4 : 0u);
  return rc;
}

int sfrt_world_check(sfrt_world* w, void* hip_stream) {
  if (!w) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  sfrt::DeviceGuard g(w->device);
  return w->read_status((hipStream_t)hip_stream);
}

int sfrt_world_trace_points(sfrt_world* w, const int32_t* ij, int count, sfrt_pixel_dump* out) {
  if (!w || count < 0 || (count > 0 && (!ij || !out))) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  int rc = w->validate();
  if (rc) return rc;
  for (int k = 0; k < count; k++)
    if (ij[2 * k] < 0 || ij[2 * k] >= w->width || ij[2 * k + 1] < 0 || ij[2 * k + 1] >= w->height)
      return SFRT_E_INVALID;
  if (count == 0) return SFRT_OK;
  static_assert(sizeof(sfrt_pixel_dump) == sizeof(sfrt::PixelDump), "dump layout");
  // The listed pixels come out of the frame-fill kernel itself (its DUMP instantiation,
  // sphere_trace.hip): a whole frame with the world's options -- the kernel table's tile
  // shape or SFRT_OPT_RAYS_PER_LANE, culling -- in the adaptive tile order when that is
  // on (three launches, so the last one runs in a sorted order), row-major otherwise.
  // Memory is O(count): the kernel binary-searches the sorted distinct pixel ids and
  // stores no frame.  The launches run on a private tile-order chain (dump_sched), so
  // the world's own chains, its last fill (sfrt_world_row_costs) and the next frame's
  // order are those of the caller's last render, untouched by the dump.
  std::vector<std::pair<int64_t, int>> ids((size_t)count);
  for (int k = 0; k < count; k++)
    ids[k] = {(int64_t)ij[2 * k + 1] * w->width + ij[2 * k], k};
  std::sort(ids.begin(), ids.end());
  std::vector<int64_t> pix;
  std::vector<int> slot((size_t)count);  // listed position -> distinct entry
  for (const auto& e : ids) {
    if (pix.empty() || pix.back() != e.first) pix.push_back(e.first);
    slot[e.second] = (int)pix.size() - 1;
  }
  sfrt::DeviceGuard g(w->device);
  sfrt::DumpArgs dump{};
  dump.npix = (int)pix.size();
  std::vector<sfrt::PixelDump> got(pix.size());
  int64_t* d_pix = nullptr;
  if (hipMalloc((void**)&d_pix, sizeof(int64_t) * pix.size()) != hipSuccess ||
      hipMalloc(&dump.out, sizeof(sfrt::PixelDump) * pix.size()) != hipSuccess) {
    (void)hipFree(d_pix);
    return SFRT_E_HIP;
  }
  dump.pix = d_pix;
  auto run = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(d_pix, pix.data(), sizeof(int64_t) * pix.size(), hipMemcpyHostToDevice,
                           w->stream));
    const int passes = w->tile_order_on ? 3 : 1;
    w->dump_sched.reset();  // this frame's own order: record, sort, use
    for (int q = 0; q < passes; q++) {
      sfrt::FrameRec f;
      std::vector<sfrt::SphereRec> recs;
      w->prepare(f, recs);
      f.xstart = 0; f.xadd = 1; f.ystart = 0; f.yadd = 1;
      f.sub_w = w->width;
      f.sub_row0 = 0;
      f.sub_rows = w->height;
      f.tiles_x = (w->width + sfrt::kTile - 1) / sfrt::kTile;
      f.out = nullptr;  // the DUMP kernels store records only
      f.out_pitch = w->width;
      int rc2 = w->stage_spheres(f, recs, w->stream, false);
      if (rc2) return rc2;
      sfrt::TileSchedPtrs p;
      if (w->tile_order_on) {
        long long tiles = 0;
        const long long key = sfrt::trace_tile_key(f, &tiles);
        HIP_TRY(w->dump_sched.begin(key, tiles, w->stream, w->tile_order_on, p));
        p.link(f);
      }
      const bool queued = sfrt::launch_trace(f, recs.data(), w->stream, &dump) == 0;
      if (w->tile_order_on) HIP_TRY(w->dump_sched.end(p, w->stream, queued));
      if (!queued) return SFRT_E_HIP;
      if ((rc2 = w->launched(w->stream))) return rc2;
    }
    HIP_TRY(hipMemcpyAsync(got.data(), dump.out, sizeof(sfrt::PixelDump) * pix.size(),
                           hipMemcpyDeviceToHost, w->stream));
    return SFRT_OK;
  };
  rc = run();
  const int st = w->read_status(w->stream);
  (void)hipFree(d_pix);
  (void)hipFree(dump.out);
  if (rc || st) return rc ? rc : st;
  for (int k = 0; k < count; k++) std::memcpy(&out[k], &got[slot[k]], sizeof(sfrt_pixel_dump));
  return SFRT_OK;
}

int sfrt_host_alloc(void** ptr, int64_t bytes) {
  if (!ptr || bytes <= 0) return SFRT_E_INVALID;
  *ptr = nullptr;
  return hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault) == hipSuccess ? SFRT_OK
                                                                               : SFRT_E_HIP;
}

int sfrt_host_free(void* ptr) {
  if (!ptr) return SFRT_OK;
  return hipHostFree(ptr) == hipSuccess ? SFRT_OK : SFRT_E_HIP;
}

int sfrt_world_submit_frame(sfrt_world* w, uint8_t* pixels, int64_t* ticket) {
  if (!w || !pixels || !ticket) return SFRT_E_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  int rc = w->validate();
  if (rc) return rc;
  sfrt::DeviceGuard g(w->device);
  if (!w->copy_stream && hipStreamCreateWithFlags(&w->copy_stream, hipStreamNonBlocking) != hipSuccess)
    return SFRT_E_HIP;
  const int64_t t = w->next_ticket;
  sfrt_world::PipeSlot& slot = w->pipe[t % sfrt_world::kPipe];
  if (!slot.rendered) {
    HIP_TRY(hipEventCreateWithFlags(&slot.rendered, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
    HIP_TRY(hipMalloc(&slot.d_status, sizeof(int)));
    HIP_TRY(hipHostMalloc(&slot.h_status, sizeof(int), hipHostMallocDefault));
  }
  const size_t px = (size_t)w->width * w->height;
  if (slot.d_buf.bytes() < px * 4) {  // stream-ordered: freed behind its last copy
    if (slot.used) HIP_TRY(hipStreamWaitEvent(w->stream, slot.copied, 0));
    HIP_TRY(slot.d_buf.reserve(px * 4, w->stream));
  }
  // The slot's previous frame must have left d_buf before this render writes it.
  if (slot.used) HIP_TRY(hipStreamWaitEvent(w->stream, slot.copied, 0));
  HIP_TRY(hipMemsetAsync(slot.d_status, 0, sizeof(int), w->stream));
  sfrt::FrameRec f;
  std::vector<sfrt::SphereRec> recs;
  const int ss = w->ss;  // supersampled: the sample frame; d_buf and the copy stay width x height
  w->prepare(f, recs, ss);
  f.xstart = 0; f.xadd = 1 << ss; f.ystart = 0; f.yadd = 1 << ss;
  f.sub_w = w->width << ss;
  f.sub_row0 = 0;
  f.sub_rows = w->height << ss;
  f.tiles_x = (f.sub_w + sfrt::kTile - 1) / sfrt::kTile;
  f.out = slot.d_buf.ptr<uint32_t>();
  f.out_pitch = w->width;
  f.status = slot.d_status;
  if ((rc = w->launchable(f))) return rc;
  rc = w->stage_spheres(f, recs, w->stream, false);
  if (rc) return rc;
  if ((rc = w->sched_begin(f, recs, w->stream))) return rc;  // adaptive tile order, as render_band
  if ((rc = w->sched_end(f, w->stream,
                         sfrt::launch_trace(f, recs.data(), w->stream, nullptr, w->ring_event(),
                                            &w->launch_caches) == 0)))
    return rc;
  if ((rc = w->launched_with())) return rc;
  HIP_TRY(hipEventRecord(slot.rendered, w->stream));
  HIP_TRY(hipStreamWaitEvent(w->copy_stream, slot.rendered, 0));
  HIP_TRY(hipMemcpyAsync(pixels, slot.d_buf.ptr(), px * 4, hipMemcpyDeviceToHost, w->copy_stream));
  HIP_TRY(hipMemcpyAsync(slot.h_status, slot.d_status, sizeof(int), hipMemcpyDeviceToHost,
                         w->copy_stream));
  HIP_TRY(hipEventRecord(slot.copied, w->copy_stream));
  slot.used = true;
  *ticket = t;
  w->next_ticket = t + 1;
  return SFRT_OK;
}

int sfrt_world_wait_frame(sfrt_world* w, int64_t ticket) {
  if (!w || ticket < 0) return SFRT_E_INVALID;
  hipEvent_t ev;
  int* h_status;
  {
    std::lock_guard<std::mutex> lk(w->mu);
    if (ticket >= w->next_ticket) return SFRT_E_INVALID;
    sfrt_world::PipeSlot& slot = w->pipe[ticket % sfrt_world::kPipe];
    // A slot reused by a newer ticket records a later event on the same
    // in-order copy stream, so waiting on it also covers this ticket.
    ev = slot.copied;
    h_status = slot.h_status;
  }
  sfrt::DeviceGuard g(w->device);
  HIP_TRY(hipEventSynchronize(ev));
  const int st = *h_status;
  if (st & 1) return SFRT_E_MARCH_LIMIT;
  if (st & 2) return SFRT_E_TEXEL;
  return SFRT_OK;
}

int sfrt_sort_spheres(sfrt_sphere* spheres, int count, const float cam_pos[3]) {
  if (count < 0 || (count > 0 && !spheres) || !cam_pos) return SFRT_E_INVALID;
  std::vector<sfrt_sphere> v(spheres, spheres + count);
  sort_spheres(v, {cam_pos[0], cam_pos[1], cam_pos[2]});
  std::memcpy(spheres, v.data(), sizeof(sfrt_sphere) * (size_t)count);
  return SFRT_OK;
}

float sfrt_deg_to_rad(float deg) { return deg * (kPI / 180.0f); }

float sfrt_pass_threshold(float radius) { return pass_threshold(radius); }

const char* sfrt_error_string(int code) {
  switch (code) {
    case SFRT_OK: return "ok";
    case SFRT_E_INVALID: return "invalid argument";
    case SFRT_E_EMPTY: return "no spheres (reference: std::out_of_range from spheres.at)";
    case SFRT_E_NO_TEXTURE: return "texture slot 0 not loaded";
    case SFRT_E_TOO_MANY: return "too many spheres";
    case SFRT_E_HIP: return "HIP runtime error";
    case SFRT_E_MARCH_LIMIT: return "march iteration limit exceeded";
    case SFRT_E_TEXEL: return "texel index outside the texture";
    default: return "unknown error";
  }
}

int sfrt_version(void) { return 18; }

const char* sfrt_build_flavour(void) { return sfrt::trace_build_flavour(); }

}  // extern "C"
