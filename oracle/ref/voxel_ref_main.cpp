// voxel_ref: runs the reference's own voxel World (its unmodified World.cpp, compiled against
// the stand-in oracle/ref/SFML/Graphics.hpp) on one request -- TEST INFRASTRUCTURE ONLY.
//
//   voxel_ref <request file> <result file>
//
// Everything is little-endian with fixed-width fields (u32, i32, f32 = IEEE binary32, u8).
// Records:  DYN   = f32 pos[3], size[2], r, g, b, distToCamera, i32 textureID        (40 bytes)
//           LIGHT = f32 pos[3], intensity, r, g, b, i32 shadows                      (32 bytes)
//           BLOCK = i32 key ((x << 20) + (y << 10) + z), i32 textureID               ( 8 bytes)
//
// Request, version 1:
//   u32 magic 0x51525856 ("VXRQ"), u32 version
//   u32 mode        0 constructor world, 1 snapshot world
//   u32 seed        what time() returns, so srand(time(NULL)) is srand(seed)
//   u32 flags       1 render a frame    2 empty `dyn` before the rays    4 rays carry their own
//                   origin (Raycast only)    8 dump the block map
//   i32 width, height
//   f32 cam_pos[3], rotation, hrotation
//   mode 0: the constructor runs, every sprite's `dir` is zeroed, the camera is assigned and
//           UpdateDyn runs twice.
//   mode 1: f32 fov_h, fov_v (radians), viewDistance, shadowDistance; u8 colors[10][4];
//           u32 n, BLOCK[n]; u32 n, DYN[n] (list order); u32 n, LIGHT[n] (`lights`);
//           u32 n, u32 index[n] (`alights` as indices into `lights`).  The constructor runs
//           first (it loads the textures); then these replace the private members.
//   u32 kind        0 no rays, 1 World::Raycast, 2 World::LRaycast
//   u32 m
//   kind 1: f32 dir[m][3], f32 yscale[m], then f32 origin[m][3] with flag 4 (assigned to
//           cam.pos before the call, the only place Raycast takes its origin from)
//   kind 2: f32 pos[m][3], f32 dir[m][3], f32 maxDist[m]
// Result, version 1:
//   u32 magic 0x53525856 ("VXRS"), u32 version
//   f32 cam_pos[3], rotation, hrotation, fov_h, fov_v, viewDistance, shadowDistance
//   u32 n, DYN[n]; u32 n, LIGHT[n]; u32 n, u32 alights index[n]     the state the frame saw
//   u32 n (0 without flag 8), BLOCK[n] sorted by key
//   u32 w, h (0, 0 without flag 1), u8 rgba[h][w][4], u8 outside[h][w]
//   u32 m, then kind 1: u8 rgba[m][4] (r->c)   kind 2: u8 free[m] (LRaycast's bool);
//   then u8 outside[m]
// `outside`: 1 where a getPixel for that pixel / ray indexed outside its image.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "ref_io.hpp"
#include "World.h"

static std::uint32_t g_seed = 0;

extern "C" time_t time(time_t* t) noexcept {
  if (t) *t = static_cast<time_t>(g_seed);
  return static_cast<time_t>(g_seed);
}

bool sf::Image::loadFromFile(const std::string& filename) {
  return refio::load_reference_image(*this, filename);
}

struct DynRec { float pos[3], size[2], r, g, b, dist; std::int32_t tex; };
struct LightRec { float pos[3], intensity, r, g, b; std::int32_t shadows; };
struct BlockRec { std::int32_t key, id; };
static_assert(sizeof(DynRec) == 40 && sizeof(LightRec) == 32 && sizeof(BlockRec) == 8, "record layout");

int main(int argc, char** argv) {
  if (argc != 3) refio::die("usage: voxel_ref <request> <result>");
  refio::Reader rq(argv[1]);
  if (rq.u32() != 0x51525856u || rq.u32() != 1u) refio::die("not a version 1 voxel request");
  const std::uint32_t mode = rq.u32();
  g_seed = rq.u32();
  const std::uint32_t flags = rq.u32();
  const std::int32_t width = rq.i32(), height = rq.i32();
  float cam[3];
  for (float& c : cam) c = rq.f32();
  const float rot = rq.f32(), hrot = rq.f32();
  if (mode > 1 || width < 0 || height < 0 || width > 4096 || height > 4096) refio::die("bad header");

  World world;  // the constructor's block map, lamps, sprites and textures
  world.cam.pos = sf::Vector3f(cam[0], cam[1], cam[2]);
  world.cam.rotation = rot;
  world.cam.hrotation = hrot;
  if (mode == 0) {
    for (Dynamic& d : world.dyn) d.dir = sf::Vector3f(0, 0, 0);
    world.UpdateDyn();
    world.UpdateDyn();
  } else {
    world.cam.fovH = rq.f32();
    world.cam.fovV = rq.f32();
    world.viewDistance = rq.f32();
    world.shadowDistance = rq.f32();
    for (int k = 0; k < 10; k++) {
      unsigned char c[4];
      rq.raw(c, 4);
      world.colors[k] = sf::Color(c[0], c[1], c[2], c[3]);
    }
    std::vector<BlockRec> blocks(rq.count(sizeof(BlockRec)));
    rq.raw(blocks.data(), blocks.size() * sizeof(BlockRec));
    std::vector<DynRec> dyn(rq.count(sizeof(DynRec)));
    rq.raw(dyn.data(), dyn.size() * sizeof(DynRec));
    std::vector<LightRec> lights(rq.count(sizeof(LightRec)));
    rq.raw(lights.data(), lights.size() * sizeof(LightRec));
    std::vector<std::uint32_t> active(rq.count(4));
    rq.raw(active.data(), active.size() * 4);
    world.blocks.clear();
    for (const BlockRec& b : blocks) {
      if (b.id < -9 || b.id > 9) refio::die("block textureID outside the ten slots");
      world.blocks.insert({b.key, Block{static_cast<short>(b.id)}});
    }
    world.dyn.clear();
    for (const DynRec& r : dyn) {
      if (r.tex < 0 || r.tex > 9) refio::die("dyn textureID outside the ten slots");
      Dynamic d;
      d.textureID = static_cast<short>(r.tex);
      d.pos = sf::Vector3f(r.pos[0], r.pos[1], r.pos[2]);
      d.size = sf::Vector2f(r.size[0], r.size[1]);
      d.distToCamera = r.dist;
      d.r = r.r; d.g = r.g; d.b = r.b;
      world.dyn.push_back(d);
    }
    world.lights.clear();
    for (const LightRec& r : lights) {
      Light l;
      l.pos = sf::Vector3f(r.pos[0], r.pos[1], r.pos[2]);
      l.intensity = r.intensity;
      l.r = r.r; l.g = r.g; l.b = r.b;
      l.shadows = r.shadows != 0;
      world.lights.push_back(l);
    }
    world.alights.clear();
    for (std::uint32_t k : active) {
      if (k >= world.lights.size()) refio::die("alights index outside lights");
      world.alights.push_back(&world.lights[k]);
    }
  }
  world.width = width;
  world.height = height;

  const std::uint32_t kind = rq.u32();
  if (kind > 2) refio::die("bad ray kind");
  const std::size_t per_ray = kind == 1 ? ((flags & 4) ? 28 : 16) : kind == 2 ? 28 : 0;
  const std::uint32_t m = per_ray ? rq.count(per_ray) : rq.u32();
  if (!per_ray && m) refio::die("rays without a kind");
  std::vector<float> a, b, c;  // kind 1: dir, yscale, origin; kind 2: pos, dir, maxDist
  if (kind == 1) {
    a.resize(static_cast<std::size_t>(m) * 3); b.resize(m); c.resize((flags & 4) ? a.size() : 0);
  } else if (kind == 2) {
    a.resize(static_cast<std::size_t>(m) * 3); b.resize(a.size()); c.resize(m);
  }
  rq.raw(a.data(), a.size() * 4);
  rq.raw(b.data(), b.size() * 4);
  rq.raw(c.data(), c.size() * 4);
  rq.done();

  refio::Writer out;
  out.u32(0x53525856u); out.u32(1);
  out.f32(world.cam.pos.x); out.f32(world.cam.pos.y); out.f32(world.cam.pos.z);
  out.f32(world.cam.rotation); out.f32(world.cam.hrotation); out.f32(world.cam.fovH); out.f32(world.cam.fovV);
  out.f32(world.viewDistance); out.f32(world.shadowDistance);
  out.u32(static_cast<std::uint32_t>(world.dyn.size()));
  for (const Dynamic& d : world.dyn) {
    const DynRec r = {{d.pos.x, d.pos.y, d.pos.z}, {d.size.x, d.size.y}, d.r, d.g, d.b, d.distToCamera, d.textureID};
    out.raw(&r, sizeof r);
  }
  out.u32(static_cast<std::uint32_t>(world.lights.size()));
  for (const Light& l : world.lights) {
    const LightRec r = {{l.pos.x, l.pos.y, l.pos.z}, l.intensity, l.r, l.g, l.b, l.shadows ? 1 : 0};
    out.raw(&r, sizeof r);
  }
  out.u32(static_cast<std::uint32_t>(world.alights.size()));
  for (const Light* l : world.alights) out.u32(static_cast<std::uint32_t>(l - world.lights.data()));
  if (flags & 8) {
    std::vector<std::pair<std::int32_t, std::int32_t>> all;
    for (const auto& kv : world.blocks) all.push_back({kv.first, kv.second.textureID});
    std::sort(all.begin(), all.end());
    out.u32(static_cast<std::uint32_t>(all.size()));
    for (const auto& kv : all) { out.i32(kv.first); out.i32(kv.second); }
  } else {
    out.u32(0);
  }

  if ((flags & 1) && width > 0 && height > 0) {
    sf::Image img;
    img.create(width, height);
    sf::standin::outside_read = 0;
    world.UpdateImage(&img, 0, 1, 0, 1);
    out.u32(width); out.u32(height);
    out.raw(img.getPixelsPtr(), static_cast<std::size_t>(width) * height * 4);
    out.raw(img.getFlagsPtr(), static_cast<std::size_t>(width) * height);
  } else {
    out.u32(0); out.u32(0);
  }

  if (flags & 2) world.dyn.clear();
  std::vector<unsigned char> answer(static_cast<std::size_t>(m) * (kind == 1 ? 4 : 1)), outside(m);
  for (std::uint32_t q = 0; q < m; q++) {
    Ray r;
    sf::standin::outside_read = 0;
    if (kind == 1) {
      if (flags & 4) world.cam.pos = sf::Vector3f(c[3 * q], c[3 * q + 1], c[3 * q + 2]);
      r.dir = sf::Vector3f(a[3 * q], a[3 * q + 1], a[3 * q + 2]);
      r.yscale = b[q];
      world.Raycast(&r);
      answer[4 * q] = r.c.r; answer[4 * q + 1] = r.c.g; answer[4 * q + 2] = r.c.b; answer[4 * q + 3] = r.c.a;
    } else {
      r.pos = sf::Vector3f(a[3 * q], a[3 * q + 1], a[3 * q + 2]);
      r.dir = sf::Vector3f(b[3 * q], b[3 * q + 1], b[3 * q + 2]);
      r.maxDist = c[q];
      answer[q] = world.LRaycast(&r) ? 1 : 0;
    }
    outside[q] = static_cast<unsigned char>(sf::standin::outside_read);
  }
  out.u32(m);
  out.raw(answer.data(), answer.size());
  out.raw(outside.data(), outside.size());
  out.save(argv[2]);
  return 0;
}
