// C++ host-side check of include/sfrt.hpp's voxel view batch: VoxelWorld::RenderViews,
// RenderViewsAux and sfrt::SortDynamics.  Built (warnings as errors) and linked against libsfrt.so
// by tests/test_voxel_views_abi.py::test_cpp_mirror_compiles_and_links.
//   cpp_voxel_views_check           SortDynamics alone: a pure host function, no device
//   cpp_voxel_views_check device    also a VoxelWorld on device 0: an empty views vector queues
//                                   nothing, a world without blocks refuses both calls with
//                                   SFRT_E_EMPTY before anything is queued or written (the targets
//                                   are never dereferenced); tests/test_voxel_views.py runs this
#include <cmath>
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

sfrt_dynamic at(float x, float y, float z) {
  sfrt_dynamic d{};
  d.pos[0] = x; d.pos[1] = y; d.pos[2] = z;
  d.size[0] = 0.15f; d.size[1] = 0.45f;
  d.r = d.g = d.b = 1.0f;
  d.dist_to_camera = 1000.0f;  // as World::AddDyn leaves it
  return d;
}

void sort_checks() {
  // distances 5 (3-4-5), 1, 5 (4-3-5), 2.5 from the camera; y is the element's identity
  std::vector<sfrt_dynamic> dyn = {at(4, 0, 6), at(2, 1, 2), at(5, 2, 5), at(1, 3, 4.5f)};
  sfrt::SortDynamics(dyn, sfrt::Vector3f{1.0f, 50.0f, 2.0f});
  const float want_dist[4] = {1.0f, 2.5f, 5.0f, 5.0f};
  const float want_id[4] = {1.0f, 3.0f, 0.0f, 2.0f};  // the tie keeps list order
  for (int k = 0; k < 4; k++) {
    expect(dyn[k].dist_to_camera == want_dist[k], "distToCamera");
    expect(dyn[k].pos[1] == want_id[k], "order");
  }
  std::vector<sfrt_dynamic> none;
  sfrt::SortDynamics(none, sfrt::Vector3f{});
  expect(none.empty(), "empty list");
  static_assert(SFRT_VOXEL_VIEWS_DYNAMICS == 1 && SFRT_MAX_VIEWS == 1024, "sfrt.h");
}

// A stereo pair with depth and cell planes, the way a caller writes it.
void stereo(sfrt::VoxelWorld& w, void* left, void* right, void* depth, void* cell, bool dynamics,
            void* stream) {
  std::vector<sfrt_view> views(2);
  views[0].cam = sfrt::to_c(w.cam);
  views[0].dev_pixels = left;
  views[1] = views[0];
  views[1].cam.pos[0] += 0.065f;
  views[1].dev_pixels = right;
  w.RenderViews(views, 4 * w.width, dynamics, stream);
  std::vector<sfrt_voxel_aux_planes> planes(2);
  planes[0].depth = depth;
  planes[0].depth_pitch_bytes = 4 * w.width;
  planes[1].cell = cell;
  planes[1].cell_pitch_bytes = 4 * w.width;
  w.RenderViewsAux(views, planes, 4 * w.width, dynamics, stream);
}

void device_checks() {
  sfrt::VoxelWorld w(0);
  w.width = 16;
  w.height = 8;
  w.RenderViews({}, 64, false, nullptr);     // nothing to queue
  w.RenderViewsAux({}, {}, 64, true, nullptr);
  // never dereferenced: a world without blocks is refused before anything is queued
  alignas(16) static uint8_t fake[4][16];
  for (bool dynamics : {false, true}) {
    int code = SFRT_OK;
    try {
      stereo(w, fake[0], fake[1], fake[2], fake[3], dynamics, nullptr);
    } catch (const sfrt::Error& e) {
      code = e.code();
    }
    expect(code == SFRT_E_EMPTY, "a world without blocks: SFRT_E_EMPTY");
  }
  int code = SFRT_OK;
  try {
    std::vector<sfrt_view> one(1);
    one[0].cam = sfrt::to_c(w.cam);
    one[0].dev_pixels = fake[0];
    w.RenderViewsAux(one, {}, 64, false, nullptr);  // one planes entry per view
  } catch (const sfrt::Error& e) {
    code = e.code();
  }
  expect(code == SFRT_E_INVALID, "planes.size() != views.size()");
  static const uint8_t zero[sizeof fake] = {};
  expect(std::memcmp(fake, zero, sizeof fake) == 0, "nothing written");
}

}  // namespace

int main(int argc, char** argv) {
  try {
    sort_checks();
    if (argc > 1 && std::strcmp(argv[1], "device") == 0) device_checks();
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    failures++;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
