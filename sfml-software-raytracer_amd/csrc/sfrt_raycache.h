// sfrt_raycache.h -- policy of the primary-ray-direction cache ("Ray cache").
//
// The normalised direction of pixel (i, j) depends only on the view basis, the ray-angle
// steps, the subset geometry and the tile grid -- not on the camera position, the spheres,
// the textures or the march.  A tile-order chain (sfrt_sched.h) whose launches keep all of
// those (RayKey) fills a tile-major buffer of directions once and reads it from then on
// (sphere_trace.hip: k_ray_fill, the CACHED kernels).  This header decides when; it makes no
// HIP call, so the policy is tested on the host (tests/native/raycache_check.cpp).  The tile
// records (TileRec, below) are filled, read and dropped by the same decisions; their layout and
// the chain's buffer bookkeeping (sfrt_hostmem.h CacheBuf) are tested in
// tests/native/tilerec_check.cpp.
#pragma once

#include <cstdint>
#include <cstring>

#include "sfrt_hostmem.h"  // CacheBuf: a chain's two buffers, for every user of this header

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

// The tile record: the other view-only part of a wave's prologue, cached beside the directions
// under the same RayKey (DESIGN.md 5 "Ray cache").  One per tile, indexed by the tile number
// sfrt_device.h slot_tile returns: the culling cone sphere_trace.hip tile_cone gives the tile
// (unit axis, sine and cosine of the half-angle, the wide flag) and the tile's column and row
// in the grid.  32 bytes, 32-byte aligned: a wave reads its record with one scalar 8-dword load
// that never straddles a 64-byte line; k_ray_fill's lane 0 writes it.
struct alignas(32) TileRec {
  float ax, ay, az;      // Cone::ax, ay, az
  float sin_t, cos_t;    // Cone::sin_t, cos_t
  uint32_t wide;         // Cone::wide (0 or 1)
  uint32_t tile_x, tile_y;
};
static_assert(sizeof(TileRec) == 32 && alignof(TileRec) == 32, "one s_load_dwordx8 per tile");

// Bytes of the records of a grid of `tiles` tiles.  They ride with the directions -- filled,
// kept and dropped with them -- and are not counted against SFRT_OPT_RAY_CACHE_MB (0.3 % of
// the directions' size at four pixels per lane, 1 % at one).
inline long long tile_rec_bytes(long long tiles) { return tiles * (long long)sizeof(TileRec); }

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
