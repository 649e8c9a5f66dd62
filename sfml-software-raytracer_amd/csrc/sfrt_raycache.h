// sfrt_raycache.h -- policy of the primary-ray-direction cache ("Ray cache").
//
// The normalised direction of pixel (i, j) depends only on the view basis, the ray-angle
// steps, the subset geometry and the tile grid -- not on the camera position, the spheres,
// the textures or the march.  A tile-order chain (sfrt_sched.h) whose launches keep all of
// those (RayKey) fills a tile-major buffer of directions once and reads it from then on
// (sphere_trace.hip: k_ray_fill, the CACHED kernels).  This header decides when; it makes no
// HIP call, so the policy is tested on the host (tests/native/raycache_check.cpp).
#pragma once

#include <cstdint>
#include <cstring>

namespace sfrt {

// Everything a cached direction depends on, as bit patterns (-0.0f and 0.0f differ, a NaN
// equals itself: the key answers "would the kernel compute the same bits", not "==").
struct RayKey {
  uint32_t fwd[3], right[3], up[3];
  uint32_t h_start, h_inc, v_start, v_inc;
  int32_t xstart, xadd, ystart, yadd, sub_w, sub_row0, sub_rows;
  long long tile_key;  // trace_tile_key: the supersampling factor, pixels per lane, the grid

  bool same(const RayKey& o) const {
    for (int q = 0; q < 3; q++)
      if (fwd[q] != o.fwd[q] || right[q] != o.right[q] || up[q] != o.up[q]) return false;
    return h_start == o.h_start && h_inc == o.h_inc && v_start == o.v_start && v_inc == o.v_inc &&
           xstart == o.xstart && xadd == o.xadd && ystart == o.ystart && yadd == o.yadd &&
           sub_w == o.sub_w && sub_row0 == o.sub_row0 && sub_rows == o.sub_rows &&
           tile_key == o.tile_key;
  }
};

inline uint32_t ray_key_bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

// Bytes of the cache of a grid of `tiles` tiles at `rays` pixels per lane: three binary32
// components per ray, clamped edge duplicates included.
inline long long ray_cache_bytes(long long tiles, int rays) { return tiles * rays * 64 * 12; }

enum class RayAction {
  kTrace,  // today's kernel; the cache is neither read nor written
  kFill,   // the fill kernel first, on the same stream, then the CACHED kernel
  kRead    // the CACHED kernel
};

// One chain's cache state.  decide() before the launch, commit() once it is known to be queued
// (or to have failed); nothing moves in between, as in TileSched.
struct RayCachePolicy {
  RayKey cached{};       // the key the buffer's contents were computed for
  bool valid = false;
  RayKey prev{};         // the previous committed launch's key
  bool have_prev = false;

  // bytes: the size the cache of `key` needs; held: the chain's own buffer size now (reused
  // or replaced by a fill); others: bytes the world's other chains hold; budget: the world's
  // limit in bytes (0: the cache is off).
  // A fill needs the second consecutive launch of a key: a camera that turns every frame
  // never fills.  A fill that would put the world past its budget is not made.
  RayAction decide(const RayKey& key, long long bytes, long long held, long long others,
                   long long budget) const {
    if (budget <= 0 || bytes <= 0) return RayAction::kTrace;
    if (valid && cached.same(key)) return RayAction::kRead;
    if (!have_prev || !prev.same(key)) return RayAction::kTrace;
    const long long after = bytes > held ? bytes : held;
    return others + after <= budget ? RayAction::kFill : RayAction::kTrace;
  }

  // queued = false: the launch (or its fill) failed -- the buffer may hold anything.
  void commit(const RayKey& key, RayAction a, bool queued) {
    if (!queued) {
      invalidate();
      return;
    }
    if (a == RayAction::kFill) {
      cached = key;
      valid = true;
    }
    prev = key;
    have_prev = true;
  }

  void invalidate() {
    valid = false;
    have_prev = false;
  }
};

}  // namespace sfrt
