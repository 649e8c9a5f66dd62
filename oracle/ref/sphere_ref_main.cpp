// sphere_ref: runs the reference's own SphereWorld (its unmodified SphereWorld.cpp, compiled
// against the stand-in oracle/ref/SFML/Graphics.hpp) on one request -- TEST INFRASTRUCTURE ONLY.
//
//   sphere_ref <request file> <result file>
//
// Everything is little-endian with fixed-width fields (u32, i32, f32 = IEEE binary32, u8).
//
// Request, version 1:
//   u32 magic 0x51524653 ("SFRQ"), u32 version
//   u32 mode        0 constructor world, 1 snapshot world
//   u32 seed        what time() returns, so srand(time(NULL)) is srand(seed)
//   u32 steps       UpdateWorld calls after the constructor (mode 0)
//   u32 flags       1 stop the camera physics before the steps (cam.airtime = 0: UpdateWorld
//                     then never calls Move, the camera stays where the constructor put it)
//                   2 assign cam.pos / rotation / hrotation after the steps (mode 0; mode 1 always)
//                   4 render a frame    8 dump the uniforms    16 rays carry their own origin
//   i32 width, height
//   f32 cam_pos[3], rotation, hrotation, fov_h, fov_v   (fov in radians; mode 1 only)
//   u32 n, f32 spheres[n][4]   x, y, z, radius in list order (mode 1; n = 0 in mode 0)
//   u32 m, f32 dirs[m][3], then f32 origins[m][3] with flag 16
// Result, version 1:
//   u32 magic 0x53524653 ("SFRS"), u32 version
//   u32 n, f32 spheres[n][4]   the `spheres` list as the frame and the rays saw it
//   f32 cam_pos[3], rotation, hrotation, fov_h, fov_v
//   u32 w, h (0, 0 without flag 4), u8 rgba[h][w][4], u8 outside[h][w]
//   u32 m, f32 pos[m][3] (r->pos), u8 rgba[m][4] (r->c), u8 outside[m]
//   u32 k (0 without flag 8), k times: u32 len, char name[len], u32 kind (0 vec4, 1 int,
//     2 float, 3 texture), f32 v[4], i32 i      -- every setUniform call, in call order
// `outside`: 1 where a getPixel for that pixel / ray indexed outside its image.
#include <cstdint>
#include <vector>

#include "ref_io.hpp"
#include "SphereWorld.h"

static std::uint32_t g_seed = 0;

extern "C" time_t time(time_t* t) noexcept {
  if (t) *t = static_cast<time_t>(g_seed);
  return static_cast<time_t>(g_seed);
}

bool sf::Image::loadFromFile(const std::string& filename) {
  return refio::load_reference_image(*this, filename);
}

int main(int argc, char** argv) {
  if (argc != 3) refio::die("usage: sphere_ref <request> <result>");
  refio::Reader rq(argv[1]);
  if (rq.u32() != 0x51524653u || rq.u32() != 1u) refio::die("not a version 1 sphere request");
  const std::uint32_t mode = rq.u32();
  g_seed = rq.u32();
  const std::uint32_t steps = rq.u32(), flags = rq.u32();
  const std::int32_t width = rq.i32(), height = rq.i32();
  float cam[3], rot, hrot, fov_h, fov_v;
  for (float& c : cam) c = rq.f32();
  rot = rq.f32(); hrot = rq.f32(); fov_h = rq.f32(); fov_v = rq.f32();
  if (mode > 1 || width < 0 || height < 0 || width > 4096 || height > 4096) refio::die("bad header");
  const std::uint32_t n = rq.count(16);
  std::vector<float> sph(static_cast<std::size_t>(n) * 4);
  rq.raw(sph.data(), sph.size() * 4);
  const std::uint32_t m = rq.count((flags & 16) ? 24 : 12);
  std::vector<float> dirs(static_cast<std::size_t>(m) * 3), org((flags & 16) ? dirs.size() : 0);
  rq.raw(dirs.data(), dirs.size() * 4);
  rq.raw(org.data(), org.size() * 4);
  rq.done();

  SphereWorld world;  // srand(seed), the constructor's AddSphere / AddLight sequence
  if (mode == 0) {
    if (flags & 1) world.cam.airtime = 0;
    for (std::uint32_t s = 0; s < steps; s++) world.UpdateWorld();
  } else {
    world.spheres.clear();
    for (std::uint32_t k = 0; k < n; k++)
      world.spheres.push_back(Sphere{sf::Vector3f(sph[4 * k], sph[4 * k + 1], sph[4 * k + 2]), sph[4 * k + 3]});
    world.cam.fovH = fov_h;
    world.cam.fovV = fov_v;
  }
  if (mode == 1 || (flags & 2)) {
    world.cam.pos = sf::Vector3f(cam[0], cam[1], cam[2]);
    world.cam.rotation = rot;
    world.cam.hrotation = hrot;
  }
  world.width = width;
  world.height = height;

  refio::Writer out;
  out.u32(0x53524653u); out.u32(1);
  out.u32(static_cast<std::uint32_t>(world.spheres.size()));
  for (const Sphere& s : world.spheres) { out.f32(s.pos.x); out.f32(s.pos.y); out.f32(s.pos.z); out.f32(s.radius); }
  out.f32(world.cam.pos.x); out.f32(world.cam.pos.y); out.f32(world.cam.pos.z);
  out.f32(world.cam.rotation); out.f32(world.cam.hrotation); out.f32(world.cam.fovH); out.f32(world.cam.fovV);
  const std::size_t uniforms_before_tracing = sf::standin::uniforms.size();

  if ((flags & 4) && width > 0 && height > 0) {
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

  std::vector<float> pos(static_cast<std::size_t>(m) * 3);
  std::vector<unsigned char> rgba(static_cast<std::size_t>(m) * 4), outside(m);
  for (std::uint32_t q = 0; q < m; q++) {
    if (flags & 16) world.cam.pos = sf::Vector3f(org[3 * q], org[3 * q + 1], org[3 * q + 2]);
    Ray r;
    r.dir = sf::Vector3f(dirs[3 * q], dirs[3 * q + 1], dirs[3 * q + 2]);
    sf::standin::outside_read = 0;
    world.Raycast(&r);
    pos[3 * q] = r.pos.x; pos[3 * q + 1] = r.pos.y; pos[3 * q + 2] = r.pos.z;
    rgba[4 * q] = r.c.r; rgba[4 * q + 1] = r.c.g; rgba[4 * q + 2] = r.c.b; rgba[4 * q + 3] = r.c.a;
    outside[q] = static_cast<unsigned char>(sf::standin::outside_read);
  }
  out.u32(m);
  out.raw(pos.data(), pos.size() * 4);
  out.raw(rgba.data(), rgba.size());
  out.raw(outside.data(), outside.size());

  if (flags & 8) {
    out.u32(static_cast<std::uint32_t>(uniforms_before_tracing));
    for (std::size_t k = 0; k < uniforms_before_tracing; k++) {
      const sf::standin::Uniform& u = sf::standin::uniforms[k];
      out.u32(static_cast<std::uint32_t>(u.name.size()));
      out.raw(u.name.data(), u.name.size());
      out.u32(static_cast<std::uint32_t>(u.kind));
      for (float v : u.v) out.f32(v);
      out.i32(u.i);
    }
  } else {
    out.u32(0);
  }
  out.save(argv[2]);
  return 0;
}
