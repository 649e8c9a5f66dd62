// C++ host-side check of include/sfrt.hpp's ray queries, written the way the reference's
// camera physics drives SphereWorld::Raycast (/root/reference/Raytracing/SphereWorld.cpp:279-289):
// rays[0].dir = (0,-1,0), rays[1].dir = (0,1,0), Raycast(rays), Raycast(&rays[1]), then the
// ground test on cam.pos.y - rays[0].pos.y.  The scene is the 10-sphere configuration
// (scenes.py default10, verbatim order) with the camera at the origin.
//  * sfrt::Ray / SphereWorld::Raycast(Ray*): r->pos and r->c of both probes equal the values
//    the caller passes (tests/raycast_ref.py's, computed by tests/test_cast_rays.py);
//  * SphereWorld::CastRays: the same two rays as one batch give the same bytes, with depth,
//    sphere and steps beside them.
// Built by tests/test_cast_rays.py (CPU: it compiles and links; GPU: it runs).
//   cpp_raycast_check <assets dir> <8 hex words: pos.x pos.y pos.z rgba of ray 0, of ray 1>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sfrt.hpp"

namespace {

uint32_t bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}
uint32_t bits(const uint8_t* c) {
  uint32_t u;
  std::memcpy(&u, c, 4);
  return u;
}

const float kDefault10[10][4] = {
    {5, 2, -4, 3}, {6, -3, -4, 2}, {-1, 2, -2, 7}, {-3, 4, 8, 2}, {-7, -3, 0, 4},
    {2, 1, 5, 7},  {-8, 4, 5, 3},  {-8, -4, 6, 3}, {-4, -2, 9, 4}, {-3, -3, -9, 5}};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  int failures = 0;
  try {
    sfrt::Image floor;
    floor.width = floor.height = 128;
    floor.pixels.resize(128 * 128 * 4);
    std::ifstream f(std::string(argv[1]) + "/floor_128x128.rgba", std::ios::binary);
    f.read(reinterpret_cast<char*>(floor.pixels.data()), (std::streamsize)floor.pixels.size());
    if (!f) throw std::runtime_error("cannot read the floor texture");
    uint32_t want[8];
    for (int k = 0; k < 8; k++) want[k] = (uint32_t)std::strtoul(argv[2 + k], nullptr, 16);

    sfrt::SphereWorld world(0);
    world.LoadTexture(floor);
    std::vector<sfrt_sphere> spheres;
    for (const auto& s : kDefault10) spheres.push_back(sfrt_sphere{s[0], s[1], s[2], s[3]});
    sfrt::check(sfrt_world_set_spheres(world.handle(), spheres.data(), (int)spheres.size()),
                "set_spheres");

    // SphereWorld.cpp:280-283
    sfrt::Ray rays[2];
    rays[0].dir = sfrt::Vector3f{0, -1, 0};
    rays[1].dir = sfrt::Vector3f{0, 1, 0};
    world.Raycast(rays);
    world.Raycast(&rays[1]);
    for (int q = 0; q < 2; q++) {
      const uint32_t got[4] = {bits(rays[q].pos.x), bits(rays[q].pos.y), bits(rays[q].pos.z),
                               bits(rays[q].c)};
      for (int k = 0; k < 4; k++)
        if (got[k] != want[4 * q + k]) {
          std::printf("Raycast: ray %d word %d: %08x, expected %08x\n", q, k, got[k], want[4 * q + k]);
          failures++;
        }
    }
    // :284-288's operands: the probe went straight down from the camera and hit below it
    if (!(rays[0].pos.x == world.cam.pos.x && rays[0].pos.z == world.cam.pos.z &&
          world.cam.pos.y - rays[0].pos.y > 0.0f && rays[1].pos.y - world.cam.pos.y > 0.0f)) {
      std::printf("Raycast: the ground probes did not move along their axis\n");
      failures++;
    }

    // the same two rays as one batch, every output
    const float dirs[6] = {0, -1, 0, 0, 1, 0};
    float pos[6], depth[2];
    int32_t sphere[2], steps[2];
    uint8_t rgba[8];
    sfrt_ray_hits out{};
    out.pos = pos; out.depth = depth; out.sphere = sphere; out.steps = steps; out.rgba = rgba;
    world.CastRays(dirs, nullptr, 2, out);
    for (int q = 0; q < 2; q++) {
      const uint32_t got[4] = {bits(pos[3 * q]), bits(pos[3 * q + 1]), bits(pos[3 * q + 2]),
                               bits(rgba + 4 * q)};
      for (int k = 0; k < 4; k++)
        if (got[k] != want[4 * q + k]) {
          std::printf("CastRays: ray %d word %d: %08x, expected %08x\n", q, k, got[k], want[4 * q + k]);
          failures++;
        }
      const float e = pos[3 * q + 1] - world.cam.pos.y;  // x and z did not move
      if (!(depth[q] == (e < 0 ? -e : e)) || sphere[q] < 0 || sphere[q] >= 10 || steps[q] < 1) {
        std::printf("CastRays: ray %d: depth %g sphere %d steps %d\n", q, depth[q], sphere[q], steps[q]);
        failures++;
      }
    }
    // an invalid ray is answered, not an error
    sfrt::Ray zero;
    world.Raycast(&zero);
    if (bits(zero.c) != 0 || zero.pos.x != 0 || zero.pos.y != 0 || zero.pos.z != 0) {
      std::printf("Raycast: a zero direction must give zeros\n");
      failures++;
    }
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    failures++;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
