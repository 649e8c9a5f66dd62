// C++ host-side check of include/sfrt.hpp's device-resident subset fill, the way the reference's
// RenderThreads refresh gameImage (Source.cpp:17-28): RenderCycles over the four column phases of
// a frame that stays in device memory, against UpdateImage of the whole frame on the host.
// Built and run by tests/test_render_subset.py::test_cpp_render_cycles.
//   cpp_subset_check <assets dir>
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sfrt.hpp"

namespace {

constexpr int kW = 45, kH = 23, kPitch = 4 * kW + 32;
constexpr uint8_t kPoison = 0xA5;

#define HIP_OK(x)                                                                  \
  do {                                                                             \
    if ((x) != hipSuccess) throw std::runtime_error(std::string("HIP: ") + #x);    \
  } while (0)

sfrt::Image load_raw(const std::string& path, int w, int h) {
  sfrt::Image img;
  img.pixels.resize((size_t)w * h * 4);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(img.pixels.data()), (std::streamsize)img.pixels.size());
  if (!f) throw std::runtime_error("cannot read " + path);
  img.width = w;
  img.height = h;
  return img;
}

struct DeviceFrame {
  void* p = nullptr;
  DeviceFrame() {
    HIP_OK(hipMalloc(&p, (size_t)kPitch * kH));
    HIP_OK(hipMemset(p, kPoison, (size_t)kPitch * kH));
    HIP_OK(hipDeviceSynchronize());
  }
  ~DeviceFrame() { (void)hipFree(p); }
  std::vector<uint8_t> read() const {
    std::vector<uint8_t> out((size_t)kPitch * kH);
    HIP_OK(hipMemcpy(out.data(), p, out.size(), hipMemcpyDeviceToHost));
    return out;
  }
};

// Pixel (i, j) of a pitched frame is all poison.
bool poisoned(const std::vector<uint8_t>& f, int i, int j) {
  for (int c = 0; c < 4; c++)
    if (f[(size_t)j * kPitch + 4 * i + c] != kPoison) return false;
  return true;
}

template <class World>
int check(World& world, const char* what) {
  int failures = 0;
  std::vector<uint8_t> host((size_t)kW * kH * 4, 0);
  world.UpdateImage(host.data(), 0, 1, 0, 1);
  hipStream_t stream;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  {  // four cycles: the whole frame, the padding untouched, cycle back at 0
    DeviceFrame frame;
    world.cycle = 0;
    world.RenderCycles(frame.p, kPitch, 4, stream);
    HIP_OK(hipStreamSynchronize(stream));
    const std::vector<uint8_t> got = frame.read();
    int bad = 0;
    for (int j = 0; j < kH; j++) {
      bad += std::memcmp(&got[(size_t)j * kPitch], &host[(size_t)j * kW * 4], 4 * kW) != 0;
      for (int b = 4 * kW; b < kPitch; b++) bad += got[(size_t)j * kPitch + b] != kPoison;
    }
    if (bad || world.cycle != 0) {
      std::printf("%s: RenderCycles(4): %d rows or padding bytes differ, cycle %d\n", what, bad,
                  world.cycle);
      failures++;
    }
  }
  {  // one cycle: column phase 0 filled, the other three poisoned, cycle == 3
    DeviceFrame frame;
    world.cycle = 0;
    world.RenderCycles(frame.p, kPitch, 1, stream);
    HIP_OK(hipStreamSynchronize(stream));
    const std::vector<uint8_t> got = frame.read();
    int bad = 0;
    for (int j = 0; j < kH; j++)
      for (int i = 0; i < kW; i++) {
        if (i % 4 == 0)
          bad += std::memcmp(&got[(size_t)j * kPitch + 4 * i], &host[((size_t)j * kW + i) * 4], 4) != 0;
        else
          bad += !poisoned(got, i, j);
      }
    if (bad || world.cycle != 3) {
      std::printf("%s: RenderCycles(1): %d pixels wrong, cycle %d\n", what, bad, world.cycle);
      failures++;
    }
  }
  HIP_OK(hipStreamDestroy(stream));
  return failures;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string assets = argv[1];
  int failures = 0;
  try {
    {
      sfrt::SphereWorld world(0);
      world.LoadTexture(load_raw(assets + "/floor_128x128.rgba", 128, 128));
      world.width = kW;
      world.height = kH;
      world.AddSphere({0, 0, 0}, 4);
      world.AddSphere({3, 1, 2}, 3);
      world.AddSphere({-2, 0.5f, 4}, 3.5f);
      world.cam.rotation = 0.7f;
      world.cam.hrotation = 0.3f;
      failures += check(world, "SphereWorld");
    }
    {
      sfrt::VoxelWorld world(0);
      // a floor, a ceiling and one wall of colour blocks around the default camera; no texture
      const int nx = 32, ny = 6, nz = 32;
      std::vector<int16_t> ids((size_t)nx * ny * nz, (int16_t)-32768);
      for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) {
          ids[((size_t)x * ny + 0) * nz + z] = -2;
          ids[((size_t)x * ny + 5) * nz + z] = -3;
          for (int y = 0; y < ny; y++)
            if (z == 20) ids[((size_t)x * ny + y) * nz + z] = (int16_t)-(1 + (x + y) % 5);
        }
      world.SetBlocks(ids, nx, ny, nz);
      world.SetColors({0, 0, 0, 255, 100, 100, 100, 255, 200, 200, 200, 255, 200, 0, 0, 255,
                       0, 200, 0, 255, 0, 0, 200, 255});
      world.SetLights({sfrt_light{{15.5f, 2.5f, 17.5f}, 2.0f, 1.0f, 1.0f, 1.0f, 1}});
      world.width = kW;
      world.height = kH;
      world.cam.rotation = 0.3f;
      failures += check(world, "VoxelWorld");
    }
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    failures++;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
