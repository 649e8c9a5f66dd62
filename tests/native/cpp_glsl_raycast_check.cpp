// C++ host-side check of include/sfrt.hpp's GLSL planes and ray queries, written the way a caller
// of the reference's shader would use them (/root/reference/Raytracing/rayShader.frag:63-179):
//  * Shader::drawImageAux: the colour equals drawImage's, and the planes say what was hit;
//  * Shader::Raycast(Ray*): the ray of fragment (i, row), set up as main() sets it up at rotation
//    (0, 0) (:172-175: dir = (ax, ay, 1), un-normalised), gives r->c == that pixel of the frame,
//    for a pixel on the light, one on an osphere and one on the wall;
//  * Shader::CastRays: the same three rays as one batch give the same colours and positions, with
//    depth, sphere and steps equal to the planes' values at those pixels, and rgba == nullptr
//    (picking) leaves those unchanged.
// The scene is built here (one wall, one light, two ospheres, a generated ground), so it needs no
// asset.  Built by tests/test_glsl_cast_rays.py (CPU: it compiles and links; GPU: it runs).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sfrt.hpp"

namespace {

uint32_t bits(const uint8_t* c) {
  uint32_t u;
  std::memcpy(&u, c, 4);
  return u;
}

constexpr int W = 40, H = 24;
constexpr float kFovX = 0.65f, kFovY = 0.41f;

}  // namespace

int main() {
  int failures = 0;
  try {
    sfrt::Shader shader(0);
    sfrt::Image ground;
    ground.width = ground.height = 64;
    ground.pixels.resize(64 * 64 * 4);
    for (int y = 0; y < 64; y++)
      for (int x = 0; x < 64; x++) {
        uint8_t* p = &ground.pixels[(size_t)(y * 64 + x) * 4];
        p[0] = (uint8_t)(x * 4); p[1] = (uint8_t)(y * 4); p[2] = (uint8_t)((x ^ y) * 4); p[3] = 255;
      }
    shader.setGround(ground);
    // spheres[]: the wall, the light, two ospheres (SphereWorld.cpp:214-238's layout)
    const sfrt::Vec4 spheres[4] = {{0, 0, 0, 8}, {0, 0, 5, 0.5f}, {2.5f, 0, 5, 1.0f}, {-2, -1, 4, 0.8f}};
    const sfrt::Vec4 lights[4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {0.5f, 1, 1, 1}, {0.5f, 1, 1, 1}};
    const sfrt::Vec4 uvs[4] = {{0.5f, 0, 0, 0}, {0.5f, 0, 0, 0}, {0.5f, 1, 0.5f, 0}, {0.5f, 1, 0.5f, 0}};
    for (int k = 0; k < 4; k++) {
      shader.setUniform("spheres[" + std::to_string(k) + "]", spheres[k]);
      shader.setUniform("lights[" + std::to_string(k) + "]", lights[k]);
      shader.setUniform("uvs[" + std::to_string(k) + "]", uvs[k]);
    }
    shader.setUniform("sphereCount", 1);
    shader.setUniform("lightCount", 1);
    shader.setUniform("allSpheresCount", 4);
    shader.setUniform("campos", sfrt::Vector3f{0, 0, 0});
    shader.setUniform("rotation", sfrt::Vector2f{0, 0});
    shader.setUniform("fov", sfrt::Vector2f{kFovX, kFovY});
    shader.setUniform("size", sfrt::Vector2f{(float)W, (float)H});

    std::vector<uint8_t> frame((size_t)W * H * 4), plain((size_t)W * H * 4);
    std::vector<float> depth((size_t)W * H);
    std::vector<int32_t> sphere((size_t)W * H), steps((size_t)W * H);
    shader.drawImageAux(frame.data(), depth.data(), sphere.data(), steps.data(), W, H);
    shader.drawImage(plain.data(), W, H);
    if (frame != plain) {
      std::printf("drawImageAux: the colour differs from drawImage's\n");
      failures++;
    }

    // main() :172-175 for fragment (i, row) at rotation (0, 0): the basis is the unit axes
    const auto pixel_ray = [&](int i, int row) {
      const float fx = (float)i + 0.5f, fy = (float)(H - 1 - row) + 0.5f;
      sfrt::Ray r;
      r.dir = sfrt::Vector3f{-kFovX + kFovX / (float)W * 2.0f * fx, -kFovY + kFovY / (float)H * 2.0f * fy, 1.0f};
      return r;
    };
    const int px[3][2] = {{20, 12}, {29, 12}, {3, 2}};  // the light, an osphere, the wall
    const int32_t want_sphere[3] = {1, 2, 0};
    float dirs[9];
    sfrt::Ray rays[3];
    for (int q = 0; q < 3; q++) {
      rays[q] = pixel_ray(px[q][0], px[q][1]);
      shader.Raycast(&rays[q]);
      const size_t p = (size_t)px[q][1] * W + px[q][0];
      if (bits(rays[q].c) != bits(&frame[p * 4]) || sphere[p] != want_sphere[q]) {
        std::printf("Raycast: pixel (%d, %d): %08x, the frame has %08x; sphere plane %d (%d)\n", px[q][0],
                    px[q][1], bits(rays[q].c), bits(&frame[p * 4]), sphere[p], want_sphere[q]);
        failures++;
      }
      dirs[3 * q] = rays[q].dir.x; dirs[3 * q + 1] = rays[q].dir.y; dirs[3 * q + 2] = rays[q].dir.z;
    }

    float pos[9], d1[3], d2[3];
    int32_t s1[3], s2[3], t1[3], t2[3];
    uint8_t rgba[12];
    sfrt_ray_hits out{};
    out.pos = pos; out.depth = d1; out.sphere = s1; out.steps = t1; out.rgba = rgba;
    shader.CastRays(dirs, 3, out);
    sfrt_ray_hits pick{};
    pick.depth = d2; pick.sphere = s2; pick.steps = t2;
    shader.CastRays(dirs, 3, pick);
    for (int q = 0; q < 3; q++) {
      const size_t p = (size_t)px[q][1] * W + px[q][0];
      const float rp[3] = {rays[q].pos.x, rays[q].pos.y, rays[q].pos.z};
      if (bits(rgba + 4 * q) != bits(rays[q].c) || std::memcmp(rp, pos + 3 * q, 12)) {
        std::printf("CastRays: ray %d: rgba %08x (Raycast %08x) or pos differs\n", q, bits(rgba + 4 * q),
                    bits(rays[q].c));
        failures++;
      }
      if (std::memcmp(&d1[q], &depth[p], 4) || s1[q] != sphere[p] || t1[q] != steps[p]) {
        std::printf("CastRays: ray %d: depth %g (%g) sphere %d (%d) steps %d (%d)\n", q, d1[q], depth[p],
                    s1[q], sphere[p], t1[q], steps[p]);
        failures++;
      }
      if (std::memcmp(&d1[q], &d2[q], 4) || s1[q] != s2[q] || t1[q] != t2[q]) {
        std::printf("CastRays: ray %d: the picking outputs differ without rgba\n", q);
        failures++;
      }
    }
    shader.Check();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    failures++;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
