// C++ host-side check of include/sfrt.hpp's voxel ray queries, written the way a World caller
// uses the reference's own signatures (/root/reference/Raytracing/World.cpp:302-491):
//  * VoxelWorld::Raycast(Ray*): the ray of pixel (i, j), set up as World::UpdateImage sets it up
//    (World.cpp:64-87: r->dir and r->yscale), gives r->c == that pixel of UpdateImage's frame, for
//    a pixel on the wall, one on the floor and one on the sky;
//  * VoxelWorld::CastRays: the same rays as one batch give the same colours, with face, cell,
//    depth and steps beside them, and rgba == nullptr (picking) leaves those unchanged;
//  * VoxelWorld::LRaycast(Ray*): true along a free segment, false through the wall, and the
//    same two answers from CastShadowRays.
// The world is built here from colour blocks (textureID < 0), so it needs no asset.
// Built by tests/test_voxel_cast_rays.py (CPU: it compiles and links; GPU: it runs).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sfrt.hpp"

namespace {

uint32_t bits(const uint8_t* c) {
  uint32_t u;
  std::memcpy(&u, c, 4);
  return u;
}

constexpr int NX = 16, NY = 8, NZ = 16, W = 101, H = 37;

}  // namespace

int main() {
  int failures = 0;
  try {
    sfrt::VoxelWorld world(0);
    world.width = W;
    world.height = H;
    std::vector<int16_t> ids((size_t)NX * NY * NZ, (int16_t)SFRT_VOXEL_EMPTY);
    for (int x = 0; x < NX; x++)
      for (int y = 0; y < NY; y++)
        for (int z = 0; z < NZ; z++)
          if (y == 0) ids[((size_t)x * NY + y) * NZ + z] = -1;        // grey floor
          else if (x == 12 && y < 5) ids[((size_t)x * NY + y) * NZ + z] = -3;  // red wall
    world.SetBlocks(ids, NX, NY, NZ);
    world.SetColors({0, 0, 0, 255, 100, 100, 100, 255, 200, 200, 200, 255, 200, 0, 0, 255});
    sfrt_light light{};
    light.pos[0] = 6.5f; light.pos[1] = 4.5f; light.pos[2] = 8.5f;
    light.intensity = 8.0f; light.r = 1.0f; light.g = 0.9f; light.b = 0.8f;
    light.shadows = 1;
    world.SetLights({light});
    world.cam.pos = {4.5f, 2.5f, 8.5f};
    world.cam.rotation = 1.5707963f;  // facing +x, the wall

    std::vector<uint8_t> frame((size_t)W * H * 4);
    world.UpdateImage(frame.data(), 0, 1, 0, 1);

    // World.cpp:64-87 for pixel (i, j)
    const auto pixel_ray = [&](int i, int j) {
      const sfrt::Camera& cam = world.cam;
      const float vStart = cam.fovV / 2, vIncreaseBy = cam.fovV / H, vOff = std::sin(cam.hrotation);
      const float hStart = cam.rotation - cam.fovH / 2, hIncreaseBy = cam.fovH / W;
      const float hray = (hStart + hIncreaseBy * i);
      const float fix = std::cos(cam.rotation - hray);
      const float vray = (vStart - j * vIncreaseBy);
      sfrt::Ray r;
      r.dir = sfrt::Vector3f{std::sin(hray) / fix, (vOff + std::sin(vray)), std::cos(hray) / fix};
      r.yscale = std::cos(cam.hrotation + vray);
      return r;
    };
    const int px[3][2] = {{50, 18}, {40, 34}, {60, 1}};  // wall, floor, above the wall
    float dirs[9], yscales[3];
    uint32_t want[3];
    for (int q = 0; q < 3; q++) {
      sfrt::Ray r = pixel_ray(px[q][0], px[q][1]);
      world.Raycast(&r);
      want[q] = bits(&frame[((size_t)px[q][1] * W + px[q][0]) * 4]);
      if (bits(r.c) != want[q]) {
        std::printf("Raycast: pixel (%d, %d): %08x, the frame has %08x\n", px[q][0], px[q][1],
                    bits(r.c), want[q]);
        failures++;
      }
      dirs[3 * q] = r.dir.x; dirs[3 * q + 1] = r.dir.y; dirs[3 * q + 2] = r.dir.z;
      yscales[q] = r.yscale;
    }
    if (want[0] == want[1] || want[0] == want[2]) {
      std::printf("the three pixels were meant to differ: %08x %08x %08x\n", want[0], want[1], want[2]);
      failures++;
    }

    float pos[9], depth[3], depth2[3];
    int32_t cell[3], face[3], steps[3], cell2[3], face2[3], steps2[3];
    uint8_t rgba[12];
    sfrt_voxel_ray_hits out{};
    out.pos = pos; out.depth = depth; out.cell = cell; out.face = face; out.steps = steps; out.rgba = rgba;
    world.CastRays(dirs, yscales, nullptr, 3, out);
    sfrt_voxel_ray_hits pick{};
    pick.depth = depth2; pick.cell = cell2; pick.face = face2; pick.steps = steps2;
    world.CastRays(dirs, yscales, nullptr, 3, pick);
    const int32_t want_face[3] = {-1, 2, 0};  // the wall's -x face, the floor's top, nothing
    for (int q = 0; q < 3; q++) {
      if (bits(rgba + 4 * q) != want[q] || face[q] != want_face[q]) {
        std::printf("CastRays: ray %d: rgba %08x (%08x) face %d (%d)\n", q, bits(rgba + 4 * q), want[q],
                    face[q], want_face[q]);
        failures++;
      }
      if (std::memcmp(&depth[q], &depth2[q], 4) || cell[q] != cell2[q] || face[q] != face2[q] ||
          steps[q] != steps2[q]) {
        std::printf("CastRays: ray %d: the picking outputs differ without rgba\n", q);
        failures++;
      }
    }
    if (cell[0] >> 20 != 12 || (cell[1] >> 10 & 1023) != 0 || cell[2] != -1 || steps[0] < 1) {
      std::printf("CastRays: cells %d %d %d steps %d\n", cell[0], cell[1], cell[2], steps[0]);
      failures++;
    }

    // line of sight: up to the light from the floor in front of the wall, and through the wall
    sfrt::Ray s;
    s.pos = sfrt::Vector3f{6.5f, 1.5f, 8.5f};
    s.dir = sfrt::Vector3f{0.0f, 1.0f, 0.0f};
    s.maxDist = 3.0f;
    const bool up = world.LRaycast(&s);
    s.dir = sfrt::Vector3f{1.0f, 0.0f, 0.0f};
    s.maxDist = 8.0f;
    const bool through = world.LRaycast(&s);
    if (!up || through) {
      std::printf("LRaycast: up %d (1), through the wall %d (0)\n", (int)up, (int)through);
      failures++;
    }
    const float org[6] = {6.5f, 1.5f, 8.5f, 6.5f, 1.5f, 8.5f}, sd[6] = {0, 1, 0, 1, 0, 0};
    const float md[2] = {3.0f, 8.0f};
    int32_t free_[2], trips[2];
    world.CastShadowRays(org, sd, md, 2, free_, trips);
    if (free_[0] != 1 || free_[1] != 0 || trips[0] < 1 || trips[1] < 1) {
      std::printf("CastShadowRays: free %d %d trips %d %d\n", free_[0], free_[1], trips[0], trips[1]);
      failures++;
    }
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    failures++;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
