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
// The cull cache (CullKey, CullCachePolicy, at the end) rides on the tile records: what each tile's
// wave culls before it marches, under a key of its own (tests/native/cullcache_check.cpp).
// The hit cache (HitRec, HitCachePolicy, after it) rides on the cull cache under the same key: what
// each ray's march leaves the shading (tests/native/hitcache_check.cpp).
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "sfrt_hostmem.h"  // CacheBuf: a chain's buffers, for every user of this header

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

// ---- The cull cache (DESIGN.md 5 "Cull cache") ----
//
// What a wave's cull (sphere_trace.hip cull_wave) leaves -- the mask m of the spheres that may
// pass for some ray of the tile and, per lane, a sphere's march window -- depends on the tile's
// cone (cached under RayKey), the camera position, the cull margin, first_l and the cull option
// (whether the wave culls at all), n, and the fields cx, cy, cz, r, s_pass of the records.  While
// all of those stay, every frame recomputes the same bits: a chain whose launches keep them
// (CullKey) fills them once (k_cull_fill) and the _cc kernels load them.  Indexed by tile number
// like TileRec, whatever the tile order.
//
// Per tile one 16-byte record, 16-byte aligned (one scalar 4-dword load): m and the tile's grid
// position, so that a reading launch loads no TileRec at all.
struct alignas(16) CullRec {
  uint32_t m_lo, m_hi;  // cull_wave's m (the list kernels: culled-list entries)
  uint32_t tile_x;
  uint32_t tile_y;      // bits 0-30; bit 31 (kCullRecFull): a list wave whose cull overflowed
                        // its 64 entries (culled == false) -- every step visits every sphere
};
static_assert(sizeof(CullRec) == 16 && alignof(CullRec) == 16, "one s_load_dwordx4 per tile");
constexpr uint32_t kCullRecFull = 0x80000000u;

// Per lane of a tile, [tile][lane]: the window of the lane's sphere (n <= 64) ...
struct alignas(8) CullWin {
  float lo, hi;
};
// ... or of the lane's culled-list entry and the entry's sphere (n > 64).
struct CullWinList {
  float lo, hi;
  int32_t cidx;
};
static_assert(sizeof(CullWin) == 8 && sizeof(CullWinList) == 12, "one vector load per lane");

inline long long cull_rec_bytes(long long tiles) { return tiles * (long long)sizeof(CullRec); }
inline long long cull_win_bytes(long long tiles, bool list) {
  return tiles * 64 * (long long)(list ? sizeof(CullWinList) : sizeof(CullWin));
}

constexpr int kCullKeyFields = 5;  // cx, cy, cz, r, s_pass

// Everything the cached bits depend on beyond the tile records, as bit patterns like RayKey.
// The record fields are a copy kept with the key and compared by value: the key relies on no
// pointer and on no promise of the caller (at most 1024 records of 20 bytes per launch).
struct CullKey {
  RayKey ray{};
  uint32_t cam[3] = {}, cull_margin = 0, first_l = 0;
  int32_t cull = 0, n = 0;
  std::vector<uint32_t> fields;  // kCullKeyFields per record, n records

  // The fields the cull reads of records recs[0..count) (any struct with SphereRec's members).
  template <class Rec>
  void set_records(const Rec* recs, int count) {
    n = count;
    fields.resize((size_t)(count > 0 ? count : 0) * kCullKeyFields);
    for (int k = 0; k < count; k++) {
      const float v[kCullKeyFields] = {recs[k].cx, recs[k].cy, recs[k].cz, recs[k].r, recs[k].s_pass};
      for (int q = 0; q < kCullKeyFields; q++) fields[(size_t)k * kCullKeyFields + q] = ray_key_bits(v[q]);
    }
  }

  bool same(const CullKey& o) const {
    if (!ray.same(o.ray) || cull != o.cull || n != o.n || cull_margin != o.cull_margin ||
        first_l != o.first_l)
      return false;
    for (int q = 0; q < 3; q++)
      if (cam[q] != o.cam[q]) return false;
    return fields == o.fields;
  }
};

// One chain's cull cache, decided after the ray cache's action for the same launch is known:
// the cull cache lives on the tile records, so it is read or filled only by a launch that reads
// the ray cache (kRead) or fills it (kFill: then the records are rewritten, and whatever the
// cull cache held is not trusted), and it is dropped with them (invalidate).  As for the
// directions, a fill needs the second consecutive launch of a key: a walking camera or a sphere
// that moves every frame never fills and runs the tile-record kernels unchanged.
struct CullCachePolicy {
  CullKey cached;
  bool valid = false;
  CullKey prev;
  bool have_prev = false;

  // ray: the ray cache's decision for this launch.  bytes: what the cull cache of `key` needs;
  // held: the chain's own cull buffers now; others: every other cached byte of the world, this
  // launch's ray cache included; budget: SFRT_OPT_RAY_CACHE_MB in bytes.
  RayAction decide(const CullKey& key, RayAction ray, long long bytes, long long held,
                   long long others, long long budget) const {
    if (budget <= 0 || bytes <= 0 || ray == RayAction::kTrace) return RayAction::kTrace;
    if (ray == RayAction::kRead && valid && cached.same(key)) return RayAction::kRead;
    if (!have_prev || !prev.same(key)) return RayAction::kTrace;
    const long long after = bytes > held ? bytes : held;
    return others + after <= budget ? RayAction::kFill : RayAction::kTrace;
  }

  // ray, a: the two decisions of the launch; queued = false: the launch or a fill failed.
  void commit(const CullKey& key, RayAction ray, RayAction a, bool queued) {
    if (!queued) {
      invalidate();
      return;
    }
    if (a == RayAction::kFill) {
      cached = key;
      valid = true;
    } else if (ray == RayAction::kFill) {
      valid = false;  // the tile records were rewritten under this cache
    }
    prev = key;
    have_prev = true;
  }

  void invalidate() {
    valid = false;
    have_prev = false;
  }
};

// ---- The hit cache (DESIGN.md 5 "Hit cache") ----
//
// The march (sphere_trace.hip march_wave) reads the rays' directions, the camera position, first_l
// and first_draw (a function of the rest), n, and the fields cx, cy, cz, r, s_pass of the records:
// exactly what CullKey holds.  What it leaves the rest of the launch is, per ray, the position and
// drawSphere, and whether the ray still moved when the trip guard ended the march (status bit 0).
// The shading tail (shade_texel) then takes the position, the camera position and the drawn
// record's cx, cy, cz, r and atan_c -- atan2f of key fields -- through two atan2f, an asinf, two
// roots and two divisions to three floats before anything of a texture enters: the fractions
// fu = u - truncf(u), u = xcoord * 4 * r, and fw = w - truncf(w), w = ycoord * 2 * r, and the
// brightness.  All of that is a function of the key too.  While the key stays, every frame repeats
// the same march and the same tail up to there: a chain whose launches keep it stores those
// results once -- from the _hf instantiation of the very kernels that march and shade, no extra
// pass -- and the reading kernels (k_shade_hits) finish the tail from them with the launch's own
// textures and texture slots, which the key does not hold: the drawn sphere's tex_off and tex_wh
// of the moment, the fractions times that size, the index, the texel, the colour.  A fraction is
// valid under every texture size; a texel index would have baked one in.
//
// Per ray one 16-byte record, 16-byte aligned, indexed by tile number like TileRec and CullRec,
// [tile][r][lane]: a wave moves 1 KiB contiguous per ray slot with one 16-byte access per lane.
// Clamped edge duplicates included; supersampled, per sample.  The three floats are stored raw,
// neither canonicalised nor packed: the reading kernel feeds the very bits into the instructions
// that follow them in the marching kernel, NaN included.
struct alignas(16) HitRec {
  uint32_t fu, fw;      // the texture coordinates' fractions, binary32 bit patterns
  uint32_t brightness;  // 3 / max(|pos - cam|, 3), binary32 bit pattern
  uint32_t draw;        // drawSphere (< n <= 1024) in the low bits; bit 31 (kHitRecMoving): the
                        // ray's last step was > 0 when march_wave returned, which only the trip
                        // guard kMaxIterations allows
};
static_assert(sizeof(HitRec) == 16 && alignof(HitRec) == 16, "one 16-byte access per ray");
constexpr uint32_t kHitRecMoving = 0x80000000u;

#if defined(__HIP__)  // the kernels' translation unit: the same helpers on both sides
#define SFRT_HIT_HD __host__ __device__ __forceinline__
#else
#define SFRT_HIT_HD inline
#endif
SFRT_HIT_HD uint32_t hit_pack_draw(int draw, bool moving) {
  return (uint32_t)draw | (moving ? kHitRecMoving : 0u);
}
SFRT_HIT_HD int hit_draw(uint32_t w) { return (int)(w & ~kHitRecMoving); }
SFRT_HIT_HD bool hit_moving(uint32_t w) { return (w & kHitRecMoving) != 0; }
SFRT_HIT_HD size_t hit_rec_at(int tile, int rays, int r, int lane) {
  return ((size_t)tile * (size_t)rays + (size_t)r) * 64u + (size_t)lane;
}
#undef SFRT_HIT_HD

inline long long hit_cache_bytes(long long tiles, int rays) {
  return tiles * rays * 64 * (long long)sizeof(HitRec);
}

// One chain's hit cache, decided after the cull cache's action for the same launch.  It is filled
// by a launch that runs the cull-cached kernel anyway (cull action kRead or kFill) on the second
// consecutive launch of a key, read by a launch that reads the cull cache under the cached key,
// and never valid without a valid cull cache: whatever refills the directions or the cull cache
// drops it.  kTrace: the launch runs what it would run without a hit cache.
struct HitCachePolicy {
  CullKey cached;
  bool valid = false;
  CullKey prev;
  bool have_prev = false;

  // cull: the cull cache's decision for this launch.  bytes: what the records of `key` need; held:
  // the chain's own hit buffer now; others: the hit bytes of the world's other chains; budget:
  // SFRT_OPT_HIT_CACHE_MB in bytes (a budget of its own).
  RayAction decide(const CullKey& key, RayAction cull, long long bytes, long long held,
                   long long others, long long budget) const {
    if (budget <= 0 || bytes <= 0 || cull == RayAction::kTrace) return RayAction::kTrace;
    if (cull == RayAction::kRead && valid && cached.same(key)) return RayAction::kRead;
    if (!have_prev || !prev.same(key)) return RayAction::kTrace;
    const long long after = bytes > held ? bytes : held;
    return others + after <= budget ? RayAction::kFill : RayAction::kTrace;
  }

  // ray, cull, a: the three decisions of the launch; queued = false: the launch or a fill failed.
  void commit(const CullKey& key, RayAction ray, RayAction cull, RayAction a, bool queued) {
    if (!queued) {
      invalidate();
      return;
    }
    if (a == RayAction::kFill) {
      cached = key;
      valid = true;
    } else if (ray == RayAction::kFill || cull == RayAction::kFill) {
      valid = false;  // the caches under this one were rewritten
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
