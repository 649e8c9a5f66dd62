// sfrt.hpp -- header-only C++ host mirror of the reference's classes over the
// C ABI (include/sfrt.h), for a drop-in at the reference's own call sites.
//
// The reference's renderers are C++ classes whose public state the caller
// mutates and whose frame fill reads it (paths under /root/reference/Raytracing/):
//   sfrt::SphereWorld  <- class SphereWorld (SphereWorld.h:40-78): width,
//                         height, cam, AddSphere, UpdateSpheres, UpdateImage
//   sfrt::MultiSphereWorld <- the same SphereWorld, its frame filled by several
//                         GPUs of the node (row bands gathered on the first one)
//   sfrt::VoxelWorld   <- class World (World.h:58-97): width, height, cam,
//                         shadowDistance, viewDistance, UpdateImage
//   sfrt::Shader       <- sf::Shader running rayShader.frag: setUniform by name,
//                         and rt.draw(sp, &shader) (Source.cpp:143-153)
// Names, argument meaning and the image orientation follow the reference.
// Errors the reference cannot report become sfrt::Error exceptions carrying
// the C ABI code (there is no silent fallback; without a HIP device the
// constructors throw).
#pragma once

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "sfrt.h"

namespace sfrt {

class Error : public std::runtime_error {
 public:
  Error(int code, const std::string& what)
      : std::runtime_error(what + ": " + sfrt_error_string(code)), code_(code) {}
  int code() const { return code_; }

 private:
  int code_;
};

inline void check(int rc, const char* what) {
  if (rc != SFRT_OK) throw Error(rc, what);
}

struct Vector2f {
  float x = 0, y = 0;
};
struct Vector3f {
  float x = 0, y = 0, z = 0;
};
struct Vec4 {  // sf::Glsl::Vec4
  float x = 0, y = 0, z = 0, w = 0;
};

// struct Camera, the fields the frame fill reads (SphereWorld.h:10-21; World.h:9-19).
struct Camera {
  Vector3f pos;
  float rotation = 0;
  float hrotation = 0;
  float fovH = 0;  // radians, as after the constructors' conversion
  float fovV = 0;
};

// sf::Image::loadFromFile for textures: PNG bytes -> RGBA8 (stb_image's 4-channel rules).
struct Image {
  std::vector<uint8_t> pixels;
  int width = 0, height = 0;
  bool loadFromMemory(const void* data, size_t size) {
    int w = 0, h = 0;
    if (sfrt_png_info(static_cast<const uint8_t*>(data), (int64_t)size, &w, &h) != SFRT_OK)
      return false;
    pixels.resize((size_t)w * h * 4);
    if (sfrt_png_decode(static_cast<const uint8_t*>(data), (int64_t)size, pixels.data(),
                        (int64_t)pixels.size(), &w, &h) != SFRT_OK)
      return false;
    width = w;
    height = h;
    return true;
  }
  bool loadFromFile(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<uint8_t> bytes;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    return loadFromMemory(bytes.data(), bytes.size());
  }
};

inline sfrt_camera to_c(const Camera& c) {
  sfrt_camera o{};
  o.pos[0] = c.pos.x;
  o.pos[1] = c.pos.y;
  o.pos[2] = c.pos.z;
  o.rotation = c.rotation;
  o.hrotation = c.hrotation;
  o.fov_h = c.fovH;
  o.fov_v = c.fovV;
  return o;
}

// struct Ray (SphereWorld.h): what SphereWorld::Raycast reads (dir) and writes (pos, c);
// c is the sf::Color's r, g, b, a.
// The voxel World's Ray (World.h:49-56) has two more members its Raycast / LRaycast read:
// yscale (the billboards' height scale) and maxDist (LRaycast's length), with its defaults.
struct Ray {
  Vector3f pos, dir;
  uint8_t c[4] = {0, 0, 0, 0};
  float maxDist = 100.0f;
  float yscale = 1.0f;
};

// ---------------------------------------------------------------------------
// SphereWorld (SphereWorld.h:40-78): the sphere-cave frame fill.
class SphereWorld {
 public:
  int width = 320;   // SphereWorld.h:50-51
  int height = 180;
  Camera cam;        // fov 75/47 degrees converted as SphereWorld.cpp:72-73

  explicit SphereWorld(int hip_device = 0) {
    check(sfrt_world_create(hip_device, &w_), "sfrt_world_create");
    sfrt_camera c;
    sfrt_world_get_camera(w_, &c);
    cam.fovH = c.fov_h;
    cam.fovV = c.fov_v;
  }
  ~SphereWorld() { sfrt_world_destroy(w_); }
  SphereWorld(const SphereWorld&) = delete;
  SphereWorld& operator=(const SphereWorld&) = delete;

  // textures[0].loadFromFile("Floor.png") (SphereWorld.cpp:52)
  void LoadTexture(const Image& img) {
    check(sfrt_world_load_texture(w_, 0, img.pixels.data(), img.width, img.height),
          "load_texture");
  }
  // SphereWorld::AddSphere (SphereWorld.cpp:177-190): containment pruning + UpdateSpheres.
  void AddSphere(Vector3f pos, float radius) {
    push_camera();
    check(sfrt_world_add_sphere(w_, pos.x, pos.y, pos.z, radius), "AddSphere");
  }
  // SphereWorld::UpdateSpheres sort (SphereWorld.cpp:199-212), against the current cam.pos.
  void UpdateSpheres() {
    push_camera();
    check(sfrt_world_update_spheres(w_), "UpdateSpheres");
  }
  std::vector<sfrt_sphere> Spheres() const {
    int n = 0;
    check(sfrt_world_get_spheres(w_, nullptr, 0, &n), "get_spheres");
    std::vector<sfrt_sphere> out((size_t)n);
    check(sfrt_world_get_spheres(w_, out.data(), n, &n), "get_spheres");
    return out;
  }
  // SphereWorld::UpdateImage (SphereWorld.cpp:83-112) into a caller-owned sf::Uint8*
  // RGBA8 frame of width*height pixels; only the addressed subset is written.
  void UpdateImage(uint8_t* pixels, short ystart, short yadd, short xstart, short xadd) {
    push_state();
    check(sfrt_world_update_image(w_, pixels, ystart, yadd, xstart, xadd), "UpdateImage");
  }
  // The same into an sf::Image-like object (setPixel(x, y, ColorT(r, g, b, a))), as the
  // reference's signature: world.UpdateImage<sf::Color>(&image, ystart, yadd, xstart, xadd).
  template <class ColorT, class ImageT>
  void UpdateImage(ImageT* v, short ystart, short yadd, short xstart, short xadd) {
    std::vector<uint8_t> frame((size_t)width * height * 4);
    UpdateImage(frame.data(), ystart, yadd, xstart, xadd);
    for (int i = xstart; i < width; i += xadd)
      for (int j = ystart; j < height; j += yadd) {
        const uint8_t* p = &frame[((size_t)j * width + i) * 4];
        v->setPixel((unsigned)i, (unsigned)j, ColorT(p[0], p[1], p[2], p[3]));
      }
  }
  // Device-resident fill of rows [row0, row0+rows) (display / multi-GPU path).
  void RenderBand(void* dev_pixels, int64_t pitch_bytes, int row0, int rows, void* hip_stream) {
    push_state();
    check(sfrt_world_render_band(w_, dev_pixels, pitch_bytes, row0, rows, hip_stream),
          "render_band");
  }
  // Both with the per-pixel planes (sfrt.h sfrt_aux_planes: hit distance before the
  // brightness clamp, drawSphere, march steps; any may be null, not all): for compositing
  // sprites behind the cave walls, picking and cost maps.
  void UpdateImageAux(uint8_t* pixels, float* depth, int32_t* sphere, int32_t* steps,
                      short ystart, short yadd, short xstart, short xadd) {
    push_state();
    check(sfrt_world_update_image_aux(w_, pixels, depth, sphere, steps, ystart, yadd, xstart, xadd),
          "UpdateImageAux");
  }
  void RenderBandAux(void* dev_pixels, int64_t pitch_bytes, const sfrt_aux_planes& aux, int row0,
                     int rows, void* hip_stream) {
    push_state();
    check(sfrt_world_render_band_aux(w_, dev_pixels, pitch_bytes, &aux, row0, rows, hip_stream),
          "render_band_aux");
  }
  // UpdateImage's subset in place in a whole width x height frame that stays in device memory
  // (sfrt.h sfrt_world_render_subset): only the addressed pixels are written; asynchronous on
  // hip_stream.  The Aux call writes the same elements of the non-null whole-frame planes.
  void UpdateImageDevice(void* dev_frame, int64_t pitch_bytes, short ystart, short yadd,
                         short xstart, short xadd, void* hip_stream) {
    push_state();
    check(sfrt_world_render_subset(w_, dev_frame, pitch_bytes, ystart, yadd, xstart, xadd, hip_stream),
          "render_subset");
  }
  void UpdateImageDeviceAux(void* dev_frame, int64_t pitch_bytes, const sfrt_aux_planes& aux,
                            short ystart, short yadd, short xstart, short xadd, void* hip_stream) {
    push_state();
    check(sfrt_world_render_subset_aux(w_, dev_frame, pitch_bytes, &aux, ystart, yadd, xstart, xadd,
                                       hip_stream),
          "render_subset_aux");
  }
  // A batch of whole frames of this world, one camera and one device target per view, in one
  // launch (sfrt.h sfrt_world_render_views): view k is the frame that `cam = views[k].cam;
  // [UpdateSpheres();] RenderBand(...)` would write, and this object's own cam and spheres are
  // left as they are.  The Aux call writes planes[k] beside view k (one entry per view).
  void RenderViews(const std::vector<sfrt_view>& views, int64_t pitch_bytes, bool sort,
                   void* hip_stream) {
    if (views.empty()) return;  // nothing to queue (an empty vector's data() may be null)
    push_state();
    check(sfrt_world_render_views(w_, views.data(), (int)views.size(), pitch_bytes,
                                  sort ? SFRT_VIEWS_SORT : 0, hip_stream),
          "render_views");
  }
  void RenderViewsAux(const std::vector<sfrt_view>& views, const std::vector<sfrt_aux_planes>& planes,
                      int64_t pitch_bytes, bool sort, void* hip_stream) {
    if (planes.size() != views.size()) throw Error(SFRT_E_INVALID, "render_views_aux");
    if (views.empty()) return;
    push_state();
    check(sfrt_world_render_views_aux(w_, views.data(), planes.data(), (int)views.size(), pitch_bytes,
                                      sort ? SFRT_VIEWS_SORT : 0, hip_stream),
          "render_views_aux");
  }
  // The reference's eight RenderThreads together (Source.cpp:17-28): each of the `cycles` steps
  // fills the columns == cycle (mod fullCycles) of every row, one launch, then steps cycle back by
  // one -- at fullCycles = 4 Source.cpp:23's (cycle + 3) % 4.  How many cycles a displayed frame
  // gets (the reference's adaptive cyclesPerFrame) is the caller's choice.
  int fullCycles = 4;
  int cycle = 0;
  void RenderCycles(void* dev_frame, int64_t pitch_bytes, int cycles, void* hip_stream) {
    for (int k = 0; k < cycles; k++) {
      UpdateImageDevice(dev_frame, pitch_bytes, 0, 1, (short)cycle, (short)fullCycles, hip_stream);
      cycle = (cycle + fullCycles - 1) % fullCycles;
    }
  }
  // SphereWorld::Raycast (SphereWorld.cpp:355-382), the reference's own signature: r->dir is
  // the un-normalised direction, the ray starts at cam.pos; writes r->pos and r->c (r->dir is
  // left as given: the normalised copy lives in the kernel).  One ray per call, synchronous:
  // the camera's ground probes (SphereWorld.cpp:279-289); batches go through CastRays.
  void Raycast(Ray* r) {
    push_camera();
    const float dir[3] = {r->dir.x, r->dir.y, r->dir.z};
    float pos[3] = {0, 0, 0};
    sfrt_ray_hits out{};
    out.pos = pos;
    out.rgba = r->c;
    check(sfrt_world_cast_rays(w_, dir, nullptr, 1, &out), "Raycast");
    r->pos = Vector3f{pos[0], pos[1], pos[2]};
  }
  // `count` rays at once (sfrt.h sfrt_world_cast_rays): dirs and origins 3 floats per ray,
  // origins null = every ray from cam.pos; any member of out may be null, not all.
  void CastRays(const float* dirs, const float* origins, int64_t count, const sfrt_ray_hits& out) {
    push_camera();
    check(sfrt_world_cast_rays(w_, dirs, origins, count, &out), "CastRays");
  }
  // The same on device memory, asynchronous on hip_stream (status through Check).
  void CastRaysDevice(const float* dev_dirs, const float* dev_origins, int64_t count,
                      const sfrt_ray_hits& dev_out, void* hip_stream) {
    push_camera();
    check(sfrt_world_cast_rays_device(w_, dev_dirs, dev_origins, count, &dev_out, hip_stream),
          "CastRaysDevice");
  }
  void Check(void* hip_stream = nullptr) { check(sfrt_world_check(w_, hip_stream), "check"); }
  // SFRT_OPT_* (sfrt.h): SFRT_OPT_SUPERSAMPLE 2 or 4 box-filters S x S samples per pixel
  // inside the frame-fill kernel; width, height and every buffer stay in output pixels.
  void SetOption(int option, int value) { check(sfrt_world_set_option(w_, option, value), "set_option"); }
  int GetOption(int option) const {
    int v = 0;
    check(sfrt_world_get_option(w_, option, &v), "get_option");
    return v;
  }
  void SetSupersample(int factor) { SetOption(SFRT_OPT_SUPERSAMPLE, factor); }
  int Supersample() const { return GetOption(SFRT_OPT_SUPERSAMPLE); }
  // SFRT_OPT_RAY_CACHE_MB (sfrt.h): MiB this world may spend on cached ray directions, 0 = off.
  void SetRayCacheMB(int mib) { SetOption(SFRT_OPT_RAY_CACHE_MB, mib); }
  int RayCacheMB() const { return GetOption(SFRT_OPT_RAY_CACHE_MB); }
  struct RayCacheStats {
    int64_t cached_frames, fills, bytes;
  };
  RayCacheStats GetRayCacheStats() const {
    RayCacheStats s{};
    check(sfrt_world_ray_cache_stats(w_, &s.cached_frames, &s.fills, &s.bytes), "ray_cache_stats");
    return s;
  }
  // Device bytes of the tile records that ride with the cached directions (sfrt.h).
  int64_t TileRecordBytes() const {
    int64_t b = 0;
    check(sfrt_world_tile_record_bytes(w_, &b), "tile_record_bytes");
    return b;
  }
  // The cull cache's counters (sfrt.h sfrt_world_cull_cache_stats).
  struct CullCacheStats {
    int64_t fills, hits, bytes;
  };
  CullCacheStats GetCullCacheStats() const {
    CullCacheStats s{};
    check(sfrt_world_cull_cache_stats(w_, &s.fills, &s.hits, &s.bytes), "cull_cache_stats");
    return s;
  }
  // SFRT_OPT_HIT_CACHE_MB (sfrt.h): MB (10^6 bytes) this world may spend on cached march results, 0 = off.
  void SetHitCacheMB(int mib) { SetOption(SFRT_OPT_HIT_CACHE_MB, mib); }
  int HitCacheMB() const { return GetOption(SFRT_OPT_HIT_CACHE_MB); }
  // The hit cache's counters (sfrt.h sfrt_world_hit_cache_stats).
  using HitCacheStats = CullCacheStats;  // the same three counters
  HitCacheStats GetHitCacheStats() const {
    HitCacheStats s{};
    check(sfrt_world_hit_cache_stats(w_, &s.fills, &s.hits, &s.bytes), "hit_cache_stats");
    return s;
  }
  // SFRT_OPT_TEXEL_CACHE (sfrt.h): the texel cache on the hit cache, under its budget; 0 = off.
  void SetTexelCache(bool on) { SetOption(SFRT_OPT_TEXEL_CACHE, on ? 1 : 0); }
  bool TexelCache() const { return GetOption(SFRT_OPT_TEXEL_CACHE) != 0; }
  // The texel cache's counters (sfrt.h sfrt_world_texel_cache_stats).
  using TexelCacheStats = CullCacheStats;  // the same three counters
  TexelCacheStats GetTexelCacheStats() const {
    TexelCacheStats s{};
    check(sfrt_world_texel_cache_stats(w_, &s.fills, &s.hits, &s.bytes), "texel_cache_stats");
    return s;
  }
  // SFRT_OPT_COMPACT_TEXELS (sfrt.h): the 4-byte compact layer on the texel cache; 0 = off, 1 = the
  // launches it was proven at (default), 2 = every eligible launch.
  void SetCompactTexels(int mode) { SetOption(SFRT_OPT_COMPACT_TEXELS, mode); }
  int CompactTexels() const { return GetOption(SFRT_OPT_COMPACT_TEXELS); }
  // The compact layer's counters (sfrt.h sfrt_world_compact_cache_stats).
  using CompactCacheStats = CullCacheStats;  // the same three counters
  CompactCacheStats GetCompactCacheStats() const {
    CompactCacheStats s{};
    check(sfrt_world_compact_cache_stats(w_, &s.fills, &s.hits, &s.bytes), "compact_cache_stats");
    return s;
  }
  // SFRT_OPT_PIXEL_CACHE (sfrt.h): the finished pixels of a scene at rest, copied until a texture
  // is loaded; 0 = off, 1 = the launches it was proven at (default), 2 = every plain band.
  void SetPixelCache(int mode) { SetOption(SFRT_OPT_PIXEL_CACHE, mode); }
  int PixelCache() const { return GetOption(SFRT_OPT_PIXEL_CACHE); }
  // The pixel layer's counters (sfrt.h sfrt_world_pixel_cache_stats).
  using PixelCacheStats = CullCacheStats;  // the same three counters
  PixelCacheStats GetPixelCacheStats() const {
    PixelCacheStats s{};
    check(sfrt_world_pixel_cache_stats(w_, &s.fills, &s.hits, &s.bytes), "pixel_cache_stats");
    return s;
  }
  sfrt_world* handle() { return w_; }

 private:
  void push_camera() {
    const sfrt_camera c = to_c(cam);
    check(sfrt_world_set_camera(w_, &c), "set_camera");
  }
  void push_state() {
    check(sfrt_world_set_size(w_, width, height), "set_size");
    push_camera();
  }
  sfrt_world* w_ = nullptr;
};

// ---------------------------------------------------------------------------
// MultiSphereWorld: SphereWorld's state and frame fill over the GPUs `devices`
// (sfrt_multi_*: row bands with global row indices, gathered on devices[0] by
// RCCL or peer copies).  UpdateImage fills the whole frame, as the reference's
// eight RenderThreads together do once per full cycle (Source.cpp:17-28).
class MultiSphereWorld {
 public:
  int width = 320;
  int height = 180;
  Camera cam;

  explicit MultiSphereWorld(const std::vector<int>& devices, int transport = SFRT_MULTI_AUTO) {
    check(sfrt_multi_create(devices.data(), (int)devices.size(), transport, &m_),
          "sfrt_multi_create");
    sfrt_world* w0 = nullptr;
    sfrt_multi_world(m_, 0, &w0);
    sfrt_camera c;
    sfrt_world_get_camera(w0, &c);
    cam.fovH = c.fov_h;
    cam.fovV = c.fov_v;
  }
  ~MultiSphereWorld() { sfrt_multi_destroy(m_); }
  MultiSphereWorld(const MultiSphereWorld&) = delete;
  MultiSphereWorld& operator=(const MultiSphereWorld&) = delete;

  void LoadTexture(const Image& img) {
    check(sfrt_multi_load_texture(m_, 0, img.pixels.data(), img.width, img.height),
          "multi_load_texture");
  }
  void AddSphere(Vector3f pos, float radius) {
    push_camera();
    check(sfrt_multi_add_sphere(m_, pos.x, pos.y, pos.z, radius), "AddSphere");
  }
  void UpdateSpheres() {
    push_camera();
    check(sfrt_multi_update_spheres(m_), "UpdateSpheres");
  }
  void SetSpheres(const std::vector<sfrt_sphere>& s) {
    check(sfrt_multi_set_spheres(m_, s.data(), (int)s.size()), "set_spheres");
  }
  // Rows per GPU (rank 0 first; empty = equal bands).
  void SetBands(const std::vector<int>& rows) {
    check(sfrt_multi_set_bands(m_, rows.empty() ? nullptr : rows.data(), (int)rows.size()),
          "set_bands");
  }
  // Cost-weighted bands from the last frame's per-row march work (sfrt_multi_balance):
  // rank 0 (no link) gets root_factor shares of the work, every other GPU one share.
  void Balance(float root_factor = 1.0f) { check(sfrt_multi_balance(m_, root_factor), "balance"); }
  // Band transfer format: SFRT_TRANSFER_AUTO (default: packed RGB + alpha bit when every
  // texel's alpha is 0 or 255), SFRT_TRANSFER_RGBA or SFRT_TRANSFER_PACKED.
  void SetTransfer(int format) { check(sfrt_multi_set_transfer(m_, format), "set_transfer"); }
  // SFRT_OPT_* on every GPU's world (sfrt_multi_set_option); read back from devices[0]'s.
  // Supersampled bands pack only when every loaded texel has one alpha (sfrt_world_alpha_binary).
  void SetOption(int option, int value) { check(sfrt_multi_set_option(m_, option, value), "set_option"); }
  int GetOption(int option) const {
    sfrt_world* w0 = nullptr;
    check(sfrt_multi_world(m_, 0, &w0), "multi_world");
    int v = 0;
    check(sfrt_world_get_option(w0, option, &v), "get_option");
    return v;
  }
  void SetSupersample(int factor) { SetOption(SFRT_OPT_SUPERSAMPLE, factor); }
  int Supersample() const { return GetOption(SFRT_OPT_SUPERSAMPLE); }
  // The whole frame into a caller-owned sf::Uint8* RGBA8 buffer (width*height*4).
  void UpdateImage(uint8_t* pixels) {
    push_state();
    check(sfrt_multi_update_image(m_, pixels), "UpdateImage");
  }
  // The whole frame into device memory on devices[0] (pitch width*4), queued after
  // hip_stream's work; complete when hip_stream passes this point.
  void Render(void* dev_frame, void* hip_stream) {
    push_state();
    check(sfrt_multi_render(m_, dev_frame, (int64_t)width * 4, hip_stream), "render");
  }
  void Check() { check(sfrt_multi_check(m_), "check"); }
  sfrt_multi* handle() { return m_; }

 private:
  void push_camera() {
    const sfrt_camera c = to_c(cam);
    check(sfrt_multi_set_camera(m_, &c), "set_camera");
  }
  void push_state() {
    check(sfrt_multi_set_size(m_, width, height), "set_size");
    push_camera();
  }
  sfrt_multi* m_ = nullptr;
};

// ---------------------------------------------------------------------------
// VoxelWorld (World.h:58-97): the voxel frame fill over a World snapshot.
class VoxelWorld {
 public:
  int width = 320;               // World.h:67-68
  int height = 180;
  Camera cam;                    // World.h:9-19 defaults, fov converted as World.cpp:55-56
  float shadowDistance = 16.0f;  // World.h:70
  float viewDistance = 24.0f;    // World.h:71

  explicit VoxelWorld(int hip_device = 0) {
    check(sfrt_voxel_create(hip_device, &v_), "sfrt_voxel_create");
    cam.pos = {15.5f, 1.9f, 15.5f};
    cam.fovH = 75.0f * (3.1415926535f / 180.0f);
    cam.fovV = 47.0f * (3.1415926535f / 180.0f);
  }
  ~VoxelWorld() { sfrt_voxel_destroy(v_); }
  VoxelWorld(const VoxelWorld&) = delete;
  VoxelWorld& operator=(const VoxelWorld&) = delete;

  void SetBlocks(const std::vector<int16_t>& ids, int nx, int ny, int nz) {
    check(sfrt_voxel_set_blocks(v_, ids.data(), nx, ny, nz), "set_blocks");
  }
  void LoadTexture(int slot, const Image& img) {
    check(sfrt_voxel_load_texture(v_, slot, img.pixels.data(), img.width, img.height),
          "load_texture");
  }
  void LoadDynTexture(int slot, const Image& img) {
    check(sfrt_voxel_load_dyn_texture(v_, slot, img.pixels.data(), img.width, img.height),
          "load_dyn_texture");
  }
  void SetColors(const std::vector<uint8_t>& rgba) {
    check(sfrt_voxel_set_colors(v_, rgba.data(), (int)(rgba.size() / 4)), "set_colors");
  }
  void SetDynamics(const std::vector<sfrt_dynamic>& dyn) {
    check(sfrt_voxel_set_dynamics(v_, dyn.data(), (int)dyn.size()), "set_dynamics");
  }
  void SetLights(const std::vector<sfrt_light>& lights) {
    check(sfrt_voxel_set_lights(v_, lights.data(), (int)lights.size()), "set_lights");
  }
  // World::UpdateImage (World.cpp:62-87) into a caller-owned RGBA8 frame.
  void UpdateImage(uint8_t* pixels, short ystart, short yadd, short xstart, short xadd) {
    push_state();
    check(sfrt_voxel_update_image(v_, pixels, ystart, yadd, xstart, xadd), "UpdateImage");
  }
  void RenderBand(void* dev_pixels, int64_t pitch_bytes, int row0, int rows, void* hip_stream) {
    push_state();
    check(sfrt_voxel_render_band(v_, dev_pixels, pitch_bytes, row0, rows, hip_stream),
          "render_band");
  }
  // The same plus the per-pixel planes (sfrt.h "the voxel frame fill's per-pixel planes"): depth,
  // cell (map key or billboard index), face (what ended Raycast) and steps; any null, not all.
  // A pick of pixel (i, j): UpdateImageAux(.., j, height, i, width).
  void UpdateImageAux(uint8_t* pixels, float* depth, int32_t* cell, int32_t* face, int32_t* steps,
                      short ystart, short yadd, short xstart, short xadd) {
    push_state();
    check(sfrt_voxel_update_image_aux(v_, pixels, depth, cell, face, steps, ystart, yadd, xstart,
                                      xadd),
          "UpdateImageAux");
  }
  void RenderBandAux(void* dev_pixels, int64_t pitch_bytes, const sfrt_voxel_aux_planes& aux,
                     int row0, int rows, void* hip_stream) {
    push_state();
    check(sfrt_voxel_render_band_aux(v_, dev_pixels, pitch_bytes, &aux, row0, rows, hip_stream),
          "render_band_aux");
  }
  // UpdateImage's subset in place in a whole width x height device frame, and the RenderThreads'
  // cycle over its column phases: as SphereWorld's (sfrt.h sfrt_voxel_render_subset).
  void UpdateImageDevice(void* dev_frame, int64_t pitch_bytes, short ystart, short yadd,
                         short xstart, short xadd, void* hip_stream) {
    push_state();
    check(sfrt_voxel_render_subset(v_, dev_frame, pitch_bytes, ystart, yadd, xstart, xadd, hip_stream),
          "render_subset");
  }
  void UpdateImageDeviceAux(void* dev_frame, int64_t pitch_bytes, const sfrt_voxel_aux_planes& aux,
                            short ystart, short yadd, short xstart, short xadd, void* hip_stream) {
    push_state();
    check(sfrt_voxel_render_subset_aux(v_, dev_frame, pitch_bytes, &aux, ystart, yadd, xstart, xadd,
                                       hip_stream),
          "render_subset_aux");
  }
  // A batch of whole frames of this world, one camera and one device target per view, in one
  // launch (sfrt.h sfrt_voxel_render_views): view k is the frame that `cam = views[k].cam;
  // [SetDynamics(SortDynamics(list, cam.pos));] RenderBand(...)` would write, and this object's own
  // cam and dynamics are left as they are.  dynamics: each view gets the list's distToCamera and
  // order for its own camera (World.cpp:226-231 at rest); without it every view walks the list as
  // it was set.  The Aux call writes planes[k] beside view k (one entry per view).
  void RenderViews(const std::vector<sfrt_view>& views, int64_t pitch_bytes, bool dynamics,
                   void* hip_stream) {
    if (views.empty()) return;  // nothing to queue (an empty vector's data() may be null)
    push_state();
    check(sfrt_voxel_render_views(v_, views.data(), (int)views.size(), pitch_bytes,
                                  dynamics ? SFRT_VOXEL_VIEWS_DYNAMICS : 0, hip_stream),
          "render_views");
  }
  void RenderViewsAux(const std::vector<sfrt_view>& views,
                      const std::vector<sfrt_voxel_aux_planes>& planes, int64_t pitch_bytes,
                      bool dynamics, void* hip_stream) {
    if (planes.size() != views.size()) throw Error(SFRT_E_INVALID, "render_views_aux");
    if (views.empty()) return;
    push_state();
    check(sfrt_voxel_render_views_aux(v_, views.data(), planes.data(), (int)views.size(), pitch_bytes,
                                      dynamics ? SFRT_VOXEL_VIEWS_DYNAMICS : 0, hip_stream),
          "render_views_aux");
  }
  int fullCycles = 4;
  int cycle = 0;
  void RenderCycles(void* dev_frame, int64_t pitch_bytes, int cycles, void* hip_stream) {
    for (int k = 0; k < cycles; k++) {
      UpdateImageDevice(dev_frame, pitch_bytes, 0, 1, (short)cycle, (short)fullCycles, hip_stream);
      cycle = (cycle + fullCycles - 1) % fullCycles;
    }
  }
  // World::Raycast (World.cpp:302-453), the reference's own signature: r->dir verbatim (never
  // normalised), r->yscale, from cam.pos with the billboards; fills r->c and r->pos (where the
  // ray ended: sfrt.h sfrt_voxel_ray_hits).  One ray per call, synchronous; batches, own
  // origins and the picking outputs (cell, face, depth) go through CastRays.
  void Raycast(Ray* r) {
    push_state();
    const float dir[3] = {r->dir.x, r->dir.y, r->dir.z};
    float pos[3] = {0, 0, 0};
    sfrt_voxel_ray_hits out{};
    out.pos = pos;
    out.rgba = r->c;
    check(sfrt_voxel_cast_rays(v_, dir, &r->yscale, nullptr, 1, &out), "Raycast");
    r->pos = Vector3f{pos[0], pos[1], pos[2]};
  }
  // World::LRaycast (World.cpp:455-491): reads r->pos, r->dir (verbatim; the reference passes a
  // normalised one) and r->maxDist; true when the segment is free.  A non-finite ray or a
  // maxDist above SFRT_VOXEL_MAX_SHADOW_DIST throws (SFRT_E_INVALID).
  bool LRaycast(Ray* r) {
    push_state();
    const float org[3] = {r->pos.x, r->pos.y, r->pos.z};
    const float dir[3] = {r->dir.x, r->dir.y, r->dir.z};
    int32_t free_ = 0;
    check(sfrt_voxel_cast_shadow_rays(v_, org, dir, &r->maxDist, 1, &free_, nullptr), "LRaycast");
    if (free_ < 0) check(SFRT_E_INVALID, "LRaycast");
    return free_ == 1;
  }
  // `count` rays at once (sfrt.h sfrt_voxel_cast_rays): dirs 3 floats per ray, yscales one (null:
  // 1.0f), origins 3 (null: every ray from cam.pos, with the billboards; given: no billboards);
  // any member of out may be null, not all.  rgba null skips the shading: the picking path.
  void CastRays(const float* dirs, const float* yscales, const float* origins, int64_t count,
                const sfrt_voxel_ray_hits& out) {
    push_state();
    check(sfrt_voxel_cast_rays(v_, dirs, yscales, origins, count, &out), "CastRays");
  }
  // The same on device memory, asynchronous on hip_stream (status through Check).
  void CastRaysDevice(const float* dev_dirs, const float* dev_yscales, const float* dev_origins,
                      int64_t count, const sfrt_voxel_ray_hits& dev_out, void* hip_stream) {
    push_state();
    check(sfrt_voxel_cast_rays_device(v_, dev_dirs, dev_yscales, dev_origins, count, &dev_out,
                                      hip_stream),
          "CastRaysDevice");
  }
  // World::LRaycast for `count` segments (sfrt.h sfrt_voxel_cast_shadow_rays): line of sight and
  // projectile tests.  free_: 1 free, 0 blocked, -1 invalid ray; steps: trips; either may be null.
  void CastShadowRays(const float* origins, const float* dirs, const float* max_dists, int64_t count,
                      int32_t* free_, int32_t* steps) {
    push_state();
    check(sfrt_voxel_cast_shadow_rays(v_, origins, dirs, max_dists, count, free_, steps),
          "CastShadowRays");
  }
  void CastShadowRaysDevice(const float* dev_origins, const float* dev_dirs, const float* dev_max_dists,
                            int64_t count, int32_t* dev_free, int32_t* dev_steps, void* hip_stream) {
    push_state();
    check(sfrt_voxel_cast_shadow_rays_device(v_, dev_origins, dev_dirs, dev_max_dists, count, dev_free,
                                             dev_steps, hip_stream),
          "CastShadowRaysDevice");
  }
  void Check(void* hip_stream = nullptr) { check(sfrt_voxel_check(v_, hip_stream), "check"); }
  // SFRT_OPT_TILE_ORDER, SFRT_OPT_SUPERSAMPLE (sfrt.h): the latter, 2 or 4, box-filters S x S
  // samples per pixel inside the kernel; width, height and every buffer stay in output pixels.
  void SetOption(int option, int value) { check(sfrt_voxel_set_option(v_, option, value), "set_option"); }
  int GetOption(int option) const {
    int v = 0;
    check(sfrt_voxel_get_option(v_, option, &v), "get_option");
    return v;
  }
  void SetSupersample(int factor) { SetOption(SFRT_OPT_SUPERSAMPLE, factor); }
  int Supersample() const { return GetOption(SFRT_OPT_SUPERSAMPLE); }

 private:
  void push_state() {
    check(sfrt_voxel_set_size(v_, width, height), "set_size");
    const sfrt_camera c = to_c(cam);
    check(sfrt_voxel_set_camera(v_, &c), "set_camera");
    check(sfrt_voxel_set_view(v_, shadowDistance, viewDistance), "set_view");
  }
  sfrt_voxel* v_ = nullptr;
};

// distToCamera and the order of a `dyn` list for a camera at rest (sfrt.h
// sfrt_voxel_sort_dynamics: stable, ascending; not the reference's one bubble pass), in place.
inline void SortDynamics(std::vector<sfrt_dynamic>& dyn, const Vector3f& cam_pos) {
  const float c[3] = {cam_pos.x, cam_pos.y, cam_pos.z};
  check(sfrt_voxel_sort_dynamics(dyn.data(), (int)dyn.size(), c), "sort_dynamics");
}

// ---------------------------------------------------------------------------
// Shader: sf::Shader with rayShader.frag loaded (SphereWorld.cpp:47), its
// setUniform calls (SphereWorld.cpp:214-238, Source.cpp:143-146) and the draw
// of a width x height render target (Source.cpp:150-153).
class Shader {
 public:
  explicit Shader(int hip_device = 0) { check(sfrt_glsl_create(hip_device, &g_), "sfrt_glsl_create"); }
  ~Shader() { sfrt_glsl_destroy(g_); }
  Shader(const Shader&) = delete;
  Shader& operator=(const Shader&) = delete;

  // setUniform("ground", texture) with setRepeated(true) + generateMipmap()
  void setGround(const Image& img) {
    check(sfrt_glsl_set_ground(g_, img.pixels.data(), img.width, img.height), "set_ground");
  }
  void setUniform(const std::string& name, float x) { set(name, &x, 1); }
  void setUniform(const std::string& name, Vector2f v) {
    const float f[2] = {v.x, v.y};
    set(name, f, 2);
  }
  void setUniform(const std::string& name, Vector3f v) {
    const float f[3] = {v.x, v.y, v.z};
    set(name, f, 3);
  }
  void setUniform(const std::string& name, Vec4 v) {
    const float f[4] = {v.x, v.y, v.z, v.w};
    set(name, f, 4);
  }
  void setUniform(const std::string& name, int v) {
    check(sfrt_glsl_set_uniform_int(g_, name.c_str(), v), name.c_str());
  }
  // rt.draw(sp, &shader) into device memory, rows [row0, row0+rows) of the target.
  void draw(void* dev_pixels, int width, int height, int64_t pitch_bytes, int row0, int rows,
            void* hip_stream) {
    check(sfrt_glsl_draw(g_, dev_pixels, width, height, pitch_bytes, row0, rows, hip_stream),
          "draw");
  }
  // rt.draw + rt.getTexture().copyToImage() into a host RGBA8 frame.
  void drawImage(uint8_t* pixels, int width, int height) {
    check(sfrt_glsl_draw_image(g_, pixels, width, height), "draw_image");
  }
  // draw plus the per-pixel planes (sfrt.h sfrt_glsl_draw_aux): depth (totalDist), sphere
  // (drawSphere) and steps (the metaball loop's trips), device memory, any of them null, not all.
  void drawAux(void* dev_pixels, int width, int height, int64_t pitch_bytes,
               const sfrt_aux_planes& aux, int row0, int rows, void* hip_stream) {
    check(sfrt_glsl_draw_aux(g_, dev_pixels, width, height, pitch_bytes, &aux, row0, rows, hip_stream),
          "draw_aux");
  }
  // drawImage plus host planes of width*height elements, any of them null, not all.
  void drawImageAux(uint8_t* pixels, float* depth, int32_t* sphere, int32_t* steps, int width,
                    int height) {
    check(sfrt_glsl_draw_image_aux(g_, pixels, depth, sphere, steps, width, height), "draw_image_aux");
  }
  // A batch of whole frames of this shader, one camera and one device target per view, in one
  // launch (sfrt.h sfrt_glsl_render_views): view k is the frame that setUniform("campos" /
  // "rotation" / "fov" from views[k].cam) + draw(...) would write, and this shader's own uniforms
  // are left as they are.  The Aux call writes planes[k] beside view k (one entry per view).
  void drawViews(const std::vector<sfrt_view>& views, int width, int height, int64_t pitch_bytes,
                 void* hip_stream) {
    if (views.empty()) return;  // nothing to queue (an empty vector's data() may be null)
    check(sfrt_glsl_render_views(g_, views.data(), (int)views.size(), width, height, pitch_bytes, 0,
                                 hip_stream),
          "render_views");
  }
  void drawViewsAux(const std::vector<sfrt_view>& views, const std::vector<sfrt_aux_planes>& planes,
                    int width, int height, int64_t pitch_bytes, void* hip_stream) {
    if (planes.size() != views.size()) throw Error(SFRT_E_INVALID, "render_views_aux");
    if (views.empty()) return;
    check(sfrt_glsl_render_views_aux(g_, views.data(), planes.data(), (int)views.size(), width,
                                     height, pitch_bytes, 0, hip_stream),
          "render_views_aux");
  }
  // The shader's Raycast(campos, r->dir, 1) (rayShader.frag:63-161) for one ray: reads r->dir
  // (un-normalised), fills r->pos and r->c.  Every ray starts at the campos uniform: r->pos is
  // not read (sfrt.h sfrt_glsl_cast_rays).  One launch and one wait per call; batches go
  // through CastRays.
  void Raycast(Ray* r) {
    const float dir[3] = {r->dir.x, r->dir.y, r->dir.z};
    float pos[3] = {0, 0, 0};
    sfrt_ray_hits out{};
    out.pos = pos;
    out.rgba = r->c;
    check(sfrt_glsl_cast_rays(g_, dir, 1, &out), "Raycast");
    r->pos = Vector3f{pos[0], pos[1], pos[2]};
  }
  // `count` rays at once: dirs 3 floats per ray; any member of out may be null, not all.
  void CastRays(const float* dirs, int64_t count, const sfrt_ray_hits& out) {
    check(sfrt_glsl_cast_rays(g_, dirs, count, &out), "CastRays");
  }
  // The same on device memory, asynchronous on hip_stream (status through Check).
  void CastRaysDevice(const float* dev_dirs, int64_t count, const sfrt_ray_hits& dev_out,
                      void* hip_stream) {
    check(sfrt_glsl_cast_rays_device(g_, dev_dirs, count, &dev_out, hip_stream), "CastRaysDevice");
  }
  void Check(void* hip_stream = nullptr) { check(sfrt_glsl_check(g_, hip_stream), "check"); }
  // SFRT_OPT_TILE_ORDER, SFRT_OPT_SUPERSAMPLE (sfrt.h): the latter, 2 or 4, box-filters the
  // fragments of the S*width x S*height target inside the kernel; draw's sizes stay in output pixels.
  void SetOption(int option, int value) { check(sfrt_glsl_set_option(g_, option, value), "set_option"); }
  int GetOption(int option) const {
    int v = 0;
    check(sfrt_glsl_get_option(g_, option, &v), "get_option");
    return v;
  }
  void SetSupersample(int factor) { SetOption(SFRT_OPT_SUPERSAMPLE, factor); }
  int Supersample() const { return GetOption(SFRT_OPT_SUPERSAMPLE); }
  sfrt_glsl* handle() { return g_; }

 private:
  void set(const std::string& name, const float* v, int n) {
    check(sfrt_glsl_set_uniform(g_, name.c_str(), v, n), name.c_str());
  }
  sfrt_glsl* g_ = nullptr;
};

}  // namespace sfrt
