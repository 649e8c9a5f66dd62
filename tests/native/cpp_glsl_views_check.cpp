// C++ host-side check of include/sfrt.hpp's GLSL view batch: Shader::drawViews and drawViewsAux.
// Built (warnings as errors) and linked against libsfrt.so by
// tests/test_glsl_views_abi.py::test_cpp_mirror_compiles_and_links.
//   cpp_glsl_views_check           the C entry points alone: a NULL shader is refused before any
//                                  device is touched
//   cpp_glsl_views_check device    also a Shader on device 0: an empty views vector queues nothing,
//                                  a shader without a ground refuses both calls with
//                                  SFRT_E_NO_TEXTURE before anything is queued or written (the
//                                  targets are never dereferenced); tests/test_glsl_views.py runs this
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sfrt.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    failures++;
  }
}

alignas(16) uint8_t fake[4][16];

sfrt_view view_at(float x, void* target) {
  sfrt_view v{};
  v.cam.pos[0] = x;
  v.cam.fov_h = 1.0f;
  v.cam.fov_v = 0.5625f;
  v.dev_pixels = target;
  return v;
}

void host_checks() {
  static_assert(SFRT_MAX_VIEWS == 1024, "sfrt.h");
  expect(sfrt_version() >= 18, "sfrt_version() >= 18");
  const sfrt_view views[2] = {view_at(0.0f, fake[0]), view_at(0.065f, fake[1])};
  sfrt_aux_planes planes[2] = {};
  planes[0].depth = fake[2];
  planes[0].depth_pitch_bytes = 16;
  planes[1].steps = fake[3];
  planes[1].steps_pitch_bytes = 16;
  expect(sfrt_glsl_render_views(nullptr, views, 2, 4, 1, 16, 0, nullptr) == SFRT_E_INVALID,
         "NULL shader");
  expect(sfrt_glsl_render_views_aux(nullptr, views, planes, 2, 4, 1, 16, 0, nullptr) == SFRT_E_INVALID,
         "NULL shader, aux");
  expect(sfrt_glsl_render_views(nullptr, views, 0, 4, 1, 16, 0, nullptr) == SFRT_E_INVALID,
         "NULL shader, count 0");
}

// A stereo pair with a depth and a steps plane, the way a caller writes it.
void stereo(sfrt::Shader& sh, int width, int height, void* stream) {
  std::vector<sfrt_view> views = {view_at(0.0f, fake[0]), view_at(0.065f, fake[1])};
  sh.drawViews(views, width, height, 4 * width, stream);
  std::vector<sfrt_aux_planes> planes(2);
  planes[0].depth = fake[2];
  planes[0].depth_pitch_bytes = 4 * width;
  planes[1].steps = fake[3];
  planes[1].steps_pitch_bytes = 4 * width;
  sh.drawViewsAux(views, planes, width, height, 4 * width, stream);
}

void device_checks() {
  sfrt::Shader sh(0);
  sh.setUniform("size", sfrt::Vector2f{4.0f, 1.0f});
  sh.drawViews({}, 4, 1, 16, nullptr);  // nothing to queue
  sh.drawViewsAux({}, {}, 4, 1, 16, nullptr);
  int code = SFRT_OK;
  try {
    stereo(sh, 4, 1, nullptr);  // never dereferenced: no ground, refused before anything is queued
  } catch (const sfrt::Error& e) {
    code = e.code();
  }
  expect(code == SFRT_E_NO_TEXTURE, "a shader without a ground: SFRT_E_NO_TEXTURE");
  code = SFRT_OK;
  try {
    sh.drawViewsAux({view_at(0.0f, fake[0])}, {}, 4, 1, 16, nullptr);  // one planes entry per view
  } catch (const sfrt::Error& e) {
    code = e.code();
  }
  expect(code == SFRT_E_INVALID, "planes.size() != views.size()");
  sh.Check(nullptr);
}

}  // namespace

int main(int argc, char** argv) {
  try {
    host_checks();
    if (argc > 1 && std::strcmp(argv[1], "device") == 0) device_checks();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    failures++;
  }
  static const uint8_t zero[sizeof fake] = {};
  expect(std::memcmp(fake, zero, sizeof fake) == 0, "nothing written");
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
