// sfrt_raycache.h -- the sphere renderer's per-chain caches ("The chain's caches").
//
// The normalised direction of pixel (i, j) depends only on the view basis, the ray-angle
// steps, the subset geometry and the tile grid -- not on the camera position, the spheres,
// the textures or the march.  A tile-order chain (sfrt_sched.h) whose launches keep all of
// those (RayKey) fills a tile-major buffer of directions and the tile records (TileRec) once
// and reads them from then on (sphere_trace.hip: k_ray_fill, the CACHED kernels).  On the tile
// records rides the cull cache (CullKey: what each tile's wave culls before it marches), and on
// that, under the same key, the hit cache (HitRec: what each ray's march leaves the shading).
// On the hit cache rides the texel cache (TexKey, TexelRec: the texel index and the brightness
// the shading is left with once the texture sizes and slots stand still too).
// On the texel cache rides the compact layer (CompactRec: the same ray in 4 bytes while the atlas
// is small enough, the brightness as its class in a table of binary32 constants).
// On top rides the pixel layer (PixelKey: the finished RGBA8 band itself while no texel changes
// either, copied into the caller's frame).
// One policy (CacheLayer) decides for each of the six; one object per chain (ChainCaches, at
// the end) owns the layers, their eight buffers and the order in which a launch decides, fills
// and drops them.  This header makes no HIP call -- the device is a parameter of
// ChainCaches::begin -- so all of it is tested on the host as it ships: tests/native/
// raycache_check.cpp (the layer), tilerec_check.cpp, cullcache_check.cpp, hitcache_check.cpp,
// texelcache_check.cpp, compactrec_check.cpp, pixelcache_check.cpp (the chain, through counting
// allocators).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
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

// One cache of a chain: the state of the directions (Key = RayKey), of the cull cache or of the hit
// cache (Key = CullKey).  decide() before the launch, commit() once it is known to be queued;
// a launch or a fill that failed goes through invalidate() -- the buffer may hold anything.
template <class Key>
struct CacheLayer {
  Key cached{};          // the key the buffer's contents were computed for
  bool valid = false;
  Key prev{};            // the previous committed launch's key
  bool have_prev = false;

  // below: this launch's decision for the layer under this one (the directions, which have
  // none: kRead) -- a layer is read only by a launch that reads the one below, and filled only
  // by one that reads or fills it.  bytes: the size the cache of `key` needs; held: the chain's
  // own buffers of this layer now (reused or replaced by a fill); others: every other byte under
  // the same budget; budget: the limit in bytes (0: off).
  // A fill needs the second consecutive launch of a key: a camera that turns every frame never
  // fills.  A fill that would put the world past its budget is not made.
  RayAction decide(const Key& key, RayAction below, long long bytes, long long held,
                   long long others, long long budget) const {
    if (budget <= 0 || bytes <= 0 || below == RayAction::kTrace) return RayAction::kTrace;
    if (below == RayAction::kRead && valid && cached.same(key)) return RayAction::kRead;
    if (!have_prev || !prev.same(key)) return RayAction::kTrace;
    const long long after = bytes > held ? bytes : held;
    return others + after <= budget ? RayAction::kFill : RayAction::kTrace;
  }

  // a: this layer's decision; below_filled: a layer under this one was rewritten by the launch.
  void commit(const Key& key, RayAction a, bool below_filled) {
    if (a == RayAction::kFill) {
      cached = key;
      valid = true;
    } else if (below_filled) {
      valid = false;
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

// ---- The texel cache (DESIGN.md 5 "Texel cache") ----
//
// What the reading kernels still compute of a HitRec every frame -- tw, th of the drawn record's
// tex_wh, tx = cvt(fu * tw), ty = cvt(fw * th), idx = tx + ty * tw, outside = !(idx < tw * th),
// tex = tex_off + idx -- depends on the record (fixed under CullKey) and on the drawn records'
// tex_off and tex_wh, and on nothing else: not on the atlas pointer and not on a texel's value.
// While those stand still too (TexKey), a ray needs 8 bytes: the texel's index in the atlas and
// the brightness.  Filled by the _tf instantiation of the k_shade_hits kernels (a launch that
// reads the hit layer anyway), read by k_shade_texels, which gathers no SphereRec at all.
//
// Per ray one 8-byte record, 8-byte aligned, indexed like HitRec: [tile][r][lane], every lane,
// clamped duplicates included, per sample when supersampled.
//   tex: Shading::tex as shade_texel leaves it (tex_off + idx), or kTexelRecOutside where the index
//     fell outside the texture.  sfrt_world_load_texture refuses an atlas above 0xffffffff texels,
//     so a valid index is at most 0xfffffffe and the sentinel is free (texel_index_fits: asserted
//     where the key is made; the layer is not filled otherwise).
//   bright: the brightness' binary32 bits with bit 31 reused for "the ray still moved at the guard"
//     (kHitRecMoving's meaning).  The brightness is 3 / max(bl, 3) with bl a correctly rounded root
//     or NaN: max(bl, 3) is >= 3 or NaN, so the quotient is in [+0, 1] or NaN -- never negative,
//     never -0 -- and its sign bit carries nothing unless it is a NaN.  A NaN's sign cannot reach
//     a byte: shade_rgba multiplies (NaN of either sign) and ends in v_cvt_u32_f32, which gives 0
//     for every NaN.  The reading kernel clears bit 31 and feeds the rest into that shade_rgba.
struct alignas(8) TexelRec {
  uint32_t tex;
  uint32_t bright;
};
static_assert(sizeof(TexelRec) == 8 && alignof(TexelRec) == 8, "one 8-byte access per ray");
constexpr uint32_t kTexelRecOutside = 0xffffffffu;
constexpr uint32_t kTexelRecMoving = 0x80000000u;

#if defined(__HIP__)
#define SFRT_TEXEL_HD __host__ __device__ __forceinline__
#else
#define SFRT_TEXEL_HD inline
#endif
SFRT_TEXEL_HD uint32_t texel_pack_tex(uint32_t tex, bool outside) { return outside ? kTexelRecOutside : tex; }
SFRT_TEXEL_HD uint32_t texel_pack_bright(uint32_t brightness_bits, bool moving) {
  return (brightness_bits & ~kTexelRecMoving) | (moving ? kTexelRecMoving : 0u);
}
SFRT_TEXEL_HD bool texel_outside(uint32_t tex) { return tex == kTexelRecOutside; }
SFRT_TEXEL_HD bool texel_moving(uint32_t bright) { return (bright & kTexelRecMoving) != 0; }
SFRT_TEXEL_HD uint32_t texel_bright_bits(uint32_t bright) { return bright & ~kTexelRecMoving; }
#undef SFRT_TEXEL_HD

inline long long texel_cache_bytes(long long tiles, int rays) {
  return tiles * rays * 64 * (long long)sizeof(TexelRec);
}
// Whether every texel index of an atlas of `texels` texels stays below the sentinel.
inline bool texel_index_fits(unsigned long long texels) { return texels <= 0xffffffffull; }

// The launch's CullKey plus tex_off and tex_wh of records 0..n-1.  Neither the atlas pointer nor a
// texel's value: a texture reloaded at its size keeps the layer; a resize, a slot change or a
// reload that shifts another slot's offset changes the key.
struct TexKey {
  CullKey cull;
  std::vector<uint32_t> tex;  // tex_off, tex_wh per record, n records

  template <class Rec>
  void set_textures(const Rec* recs, int count) {
    tex.resize((size_t)(count > 0 ? count : 0) * 2);
    for (int k = 0; k < count; k++) {
      tex[(size_t)k * 2] = recs[k].tex_off;
      tex[(size_t)k * 2 + 1] = recs[k].tex_wh;
    }
  }
  bool same(const TexKey& o) const { return tex == o.tex && cull.same(o.cull); }
};

// ---- The compact layer (DESIGN.md 5 "Compact layer") ----
//
// A TexelRec holds more than a pixel needs.  shade_rgba uses the brightness b only in
// cvt_u32(float(c) * b) for the three channel bytes c in 0..255; each is monotone in b, and b is
// 3 / max(bl, 3): in [+0, 1] or NaN, a NaN giving 0 for every c as b = 0 does.  Two brightnesses
// with the same 256 results are interchangeable byte for byte under every texel, and the classes
// are intervals of b: their lower ends are, for c in 1..255 and k in 1..c, the smallest binary32 t
// with cvt_u32(fl(c * t)) >= k -- at most 32,640 of them, 20,228 distinct in binary32 (thresholds
// k/c and 2k/2c that rounding splits by an ulp included), so a class fits 15 bits.  With an atlas
// of at most 0xffff texels the index fits 16, and a ray fits one dword.
//
// Per ray one 4-byte record, [tile][lane][r] -- the reading kernel's lane owns R consecutive
// pixels of one row (sphere_trace.hip k_shade_compact) and loads its R records with one access --
// every slot written, clamped duplicates included.
//   bits 0-15: Shading::tex, or kCompactOutside where the index fell outside the texture
//   bits 16-30: the brightness' class (BrightClasses::class_of)
//   bit 31: kTexelRecMoving's meaning
struct CompactRec {
  uint32_t w;
};
static_assert(sizeof(CompactRec) == 4 && alignof(CompactRec) == 4, "one dword per ray");
constexpr uint32_t kCompactOutside = 0xffffu;
constexpr uint32_t kCompactMoving = 0x80000000u;
constexpr uint32_t kCompactClassLimit = 1u << 15;  // classes a record can name

#if defined(__HIP__)
#define SFRT_COMPACT_HD __host__ __device__ __forceinline__
#else
#define SFRT_COMPACT_HD inline
#endif
SFRT_COMPACT_HD uint32_t compact_pack(uint32_t tex, bool outside, uint32_t cls, bool moving) {
  return (outside ? kCompactOutside : (tex & 0xffffu)) | ((cls & (kCompactClassLimit - 1u)) << 16) |
         (moving ? kCompactMoving : 0u);
}
SFRT_COMPACT_HD uint32_t compact_tex(uint32_t w) { return w & 0xffffu; }
SFRT_COMPACT_HD bool compact_outside(uint32_t w) { return (w & 0xffffu) == kCompactOutside; }
SFRT_COMPACT_HD uint32_t compact_class(uint32_t w) { return (w >> 16) & (kCompactClassLimit - 1u); }
SFRT_COMPACT_HD bool compact_moving(uint32_t w) { return (w & kCompactMoving) != 0; }
SFRT_COMPACT_HD size_t compact_rec_at(int tile, int rays, int lane, int r) {
  return ((size_t)tile * 64u + (size_t)lane) * (size_t)rays + (size_t)r;
}
// The class of a brightness, given as its binary32 bits with bit 31 clear, in the table rep[0 ..
// classes): 0 for a NaN, else the number of thresholds rep[1 .. classes) that are <= b.  Unsigned
// compares of the bit patterns, exact because b >= +0; fifteen steps whatever the table's size
// (classes <= kCompactClassLimit).  The device searches the uploaded table with this very function:
// no arithmetic decides a class.
SFRT_COMPACT_HD uint32_t bright_class_of(const uint32_t* rep, uint32_t classes, uint32_t b) {
  if (b > 0x7f800000u) return 0u;  // NaN (the sign is not part of b)
  uint32_t cls = 0;                // rep[0] = +0 <= b
  for (uint32_t step = kCompactClassLimit >> 1; step; step >>= 1) {
    const uint32_t m = cls + step;
    if (m < classes && rep[m] <= b) cls = m;
  }
  return cls;
}
#undef SFRT_COMPACT_HD

inline long long compact_cache_bytes(long long tiles, int rays) {
  return tiles * rays * 64 * (long long)sizeof(CompactRec);
}
// Whether every texel index of an atlas of `texels` texels stays below kCompactOutside.
inline bool compact_index_fits(unsigned long long texels) { return texels <= 0xffffull; }
// The largest tex_off + tw * th over records recs[0..count) (any struct with SphereRec's members):
// one past the last texel index a ray of the launch can be left with.  A function of the TexKey's
// fields, computed where the key is made.
template <class Rec>
unsigned long long compact_texel_end(const Rec* recs, int count) {
  unsigned long long end = 0;
  for (int k = 0; k < count; k++) {
    const unsigned long long e = (unsigned long long)recs[k].tex_off +
                                 (unsigned long long)(recs[k].tex_wh & 0xffffu) * (recs[k].tex_wh >> 16);
    if (e > end) end = e;
  }
  return end;
}
// The layer's own eligibility condition: no supersampling (ss: log2 of the factor) and every index
// in 16 bits.
template <class Rec>
bool compact_eligible(const Rec* recs, int count, int ss) {
  return ss == 0 && compact_index_fits(compact_texel_end(recs, count));
}

// shade_rgba's channel (sphere_trace.hip) on the host: one rounding for the product -- this header
// is compiled with -ffp-contract=off wherever the result matters, and a lone product has nothing to
// contract with -- then v_cvt_u32_f32: towards zero, 0 for a NaN.  b in [+0, 1] or NaN.
inline uint32_t bright_channel(uint32_t c, float b) {
  const volatile float p = (float)c * b;  // (volatile: binary32, not an x87 temporary)
  return p != p ? 0u : (uint32_t)p;
}
inline uint32_t bright_shade_rgba(uint32_t texel, float b) {
  return (bright_channel(texel & 0xffu, b) & 0xffu) | ((bright_channel((texel >> 8) & 0xffu, b) & 0xffu) << 8) |
         ((bright_channel((texel >> 16) & 0xffu, b) & 0xffu) << 16) | (texel & 0xff000000u);
}

// The class table, a constant of binary32 arithmetic: rep[i] is class i's smallest brightness
// (rep[0] = +0), as bit patterns, strictly increasing.  Built once per process.
struct BrightClasses {
  std::vector<uint32_t> rep;

  static float from_bits(uint32_t u) {
    float v;
    std::memcpy(&v, &u, 4);
    return v;
  }
  static BrightClasses make() {
    BrightClasses t;
    std::vector<uint32_t> thr;
    thr.reserve(255 * 128);
    for (uint32_t c = 1; c <= 255; c++) {
      for (uint32_t k = 1; k <= c; k++) {
        // the smallest t with cvt(fl(c * t)) >= k: positive floats order as their bits do
        uint32_t u = ray_key_bits((float)k / (float)c);
        while (bright_channel(c, from_bits(u)) < k) u++;
        while (bright_channel(c, from_bits(u - 1)) >= k) u--;
        thr.push_back(u);
      }
    }
    std::sort(thr.begin(), thr.end());
    thr.erase(std::unique(thr.begin(), thr.end()), thr.end());
    t.rep.reserve(thr.size() + 1);
    t.rep.push_back(0u);
    t.rep.insert(t.rep.end(), thr.begin(), thr.end());
    return t;
  }
  static const BrightClasses& get() {
    static const BrightClasses t = make();
    return t;
  }
  uint32_t classes() const { return (uint32_t)rep.size(); }
  // a record can name every class (else the layer is never filled)
  bool fits() const { return !rep.empty() && rep.size() < kCompactClassLimit; }
  uint32_t class_of(float b) const {
    return bright_class_of(rep.data(), classes(), ray_key_bits(b) & ~kCompactMoving);
  }
};

// ---- The pixel layer (DESIGN.md 5 "Pixel layer") ----
//
// What a launch that shades from the texel or the compact records still computes of a ray every
// frame -- the texel gather, rep[class], shade_rgba, the box filter when supersampled -- depends on
// the records (fixed under TexKey) and on the atlas' texels, and on nothing else.  Texels reach the
// atlas only through the library (sfrt_world_load_texture), which counts every such call in a
// per-world generation: while the TexKey and the generation stand still (PixelKey), a plain
// render_band launch is a copy of the band it wrote the last time.
//
// The band's output pixels, after the box filter: sub_w >> ss columns by sub_rows >> ss rows of
// RGBA8, rows packed in frame order, no tiles, the buffer 16-byte aligned (an allocation's start).
// The band's rows and width and the supersampling factor are the RayKey's (sub_row0, sub_rows,
// sub_w, tile_key bits 59-60); the caller's base and pitch are no part of the key -- the copy
// kernel (sphere_trace.hip k_pixels_copy) takes them from the launch.
// The launch's status bits (the values 1, the march guard hit, and 2, a texel outside its texture) are constants of the key too: the filling
// launch raises them in a word the layer owns, and every copy ORs that word into the world's.
inline long long pixel_cache_bytes(long long out_w, long long out_rows) { return out_w * out_rows * 4; }

struct PixelKey {
  TexKey tex;
  unsigned long long generation = 0;  // the world's count of atlas writes
  bool same(const PixelKey& o) const { return generation == o.generation && tex.same(o.tex); }
};

// ---- One chain's caches (DESIGN.md 5 "The chain's caches") ----

// What ChainCaches::begin decided for one launch and what that launch reads: launch_trace's cache
// argument (sfrt_trace.h).  A pointer is set exactly when its layer's action is not kTrace.
struct TraceCaches {
  bool decided = false;  // begin() made it: end() has something to commit
  RayAction ray = RayAction::kTrace, cull = RayAction::kTrace, hit = RayAction::kTrace;
  RayAction texel = RayAction::kTrace;  // kRead implies hit == kRead; kFill rides on a hit read
  RayAction compact = RayAction::kTrace;  // kRead implies texel == kRead; kFill rides on a texel read
  // kRead: the launch is one copy of pixels into the caller's band (the decisions under it stay
  // kRead: it counts as a read of theirs); kFill: the launch the layers under it decided, into the
  // caller's band with the layer's status word for the world's, then a copy of the band into pixels
  RayAction pixel = RayAction::kTrace;
  const float* dirs = nullptr;
  const TileRec* tile_recs = nullptr;
  const CullRec* cull_recs = nullptr;
  const void* cull_wins = nullptr;  // CullWin or CullWinList
  HitRec* hit_recs = nullptr;       // written by a filling launch (hit == kFill), read by a reading one
  TexelRec* texel_recs = nullptr;   // likewise (a launch that reads them still gets hit_recs, unread)
  CompactRec* compact_recs = nullptr;  // likewise (a launch that reads them still gets texel_recs, unread)
  uint32_t* pixels = nullptr;          // set exactly when pixel != kTrace
  // the layer's status word on the device, set by the caller of begin() for a launch whose pixel
  // action is not kTrace: zeroed and raised by the filling launch, ORed into the world's by every copy
  int* pixel_status = nullptr;
  // the world's class table on the device (BrightClasses::rep), set by the caller of begin() for a
  // launch whose compact action is not kTrace; readable up to kCompactClassLimit entries
  const uint32_t* bright_rep = nullptr;
  uint32_t bright_classes = 0;
  bool reading() const { return hit == RayAction::kRead; }  // no march: outside the tile order
};

struct CacheSizes {  // of one launch's grid: ray_cache_bytes, tile_rec_bytes, cull_*_bytes, hit_cache_bytes
  long long dirs = 0, tile_recs = 0, cull_recs = 0, cull_wins = 0, hit_recs = 0;
  long long texel_recs = 0;  // texel_cache_bytes (0: no texel layer)
  long long compact_recs = 0;  // compact_cache_bytes (0: no compact layer, or the launch is not eligible)
  long long pixels = 0;  // pixel_cache_bytes (0: no pixel layer)
};

struct CacheCounters {  // sfrt_world_{ray,cull,hit,texel}_cache_stats
  int64_t ray_cached_frames = 0, ray_fills = 0, cull_fills = 0, cull_hits = 0, hit_fills = 0, hit_hits = 0;
  int64_t texel_fills = 0, texel_hits = 0;
  int64_t compact_fills = 0, compact_hits = 0;
  int64_t pixel_fills = 0, pixel_hits = 0;
};

// The six layers and the eight buffers of one tile-order chain, and the one rule between them:
// an upper cache is never valid without the one under it.  A refill below drops what is above; a
// failed fill drops its own layer and everything above it; a failed launch drops all six.
// The texel layer (TexKey) has no fill kernel of its own and is not filled by a marching launch:
// only a launch that reads the hit layer fills it (the _tf kernels), and a launch that reads it
// counts as a read of the three layers under it.
// The compact layer (TexKey again; eligible: begin's compact_ok) likewise one step up: only a launch
// that reads the texel layer fills it (k_shade_texels_cf), a launch that reads it counts as a read
// of the four under it, and whatever drops or refills the texel layer frees its buffer first, so it
// never takes room a lower layer could have had in this chain.
// The pixel layer (PixelKey; begin's pixel_generation) rides on the topmost of those two the launch
// has: only a launch that reads the compact layer -- or the texel layer, where no compact layer is
// decided for it -- fills it (its band copied behind it), a launch that reads it counts as a read of
// every layer under it, and whatever drops or refills one of them frees its buffer first.
struct ChainCaches {
  CacheLayer<RayKey> ray;
  CacheLayer<CullKey> cull, hit;
  CacheLayer<TexKey> texel, compact;
  CacheLayer<PixelKey> pixel;
  CacheBuf dirs, tile_recs;  // ray_cache_bytes, tile_rec_bytes: one layer, two buffers
  CacheBuf cull_recs, cull_wins;
  CacheBuf hit_recs;
  CacheBuf texel_recs;
  CacheBuf compact_recs;
  CacheBuf pixels;
  RayKey ray_key{};  // begin() -> end(): the launch being queued
  CullKey cull_key;
  TexKey tex_key;
  bool have_tex_key = false;
  PixelKey pixel_key;  // (its .tex assigned only for a launch with a pixel layer)
  bool have_pixel_key = false;

  long long cull_bytes() const { return cull_recs.bytes + cull_wins.bytes; }
  // What SFRT_OPT_RAY_CACHE_MB limits (the tile records ride free: 0.3 to 1 % of the directions),
  // what SFRT_OPT_HIT_CACHE_MB limits, and the tile records, reported on their own.
  long long bytes_under_ray_budget() const { return dirs.bytes + cull_bytes(); }
  long long hit_bytes() const { return hit_recs.bytes; }  // the hit records alone (the stats)
  long long texel_bytes() const { return texel_recs.bytes; }
  long long compact_bytes() const { return compact_recs.bytes; }
  long long pixel_bytes() const { return pixels.bytes; }
  long long bytes_under_hit_budget() const {
    return hit_recs.bytes + texel_recs.bytes + compact_recs.bytes + pixels.bytes;
  }
  long long tile_rec_bytes() const { return tile_recs.bytes; }

  // Before a launch that takes part.  other_ray, other_hit: what the world's other chains hold
  // under the two budgets.  dev: the device in the launch's stream order -- free(p) -> bool,
  // alloc(n) -> pointer or null, fill_rays(dirs, tile_recs) -> bool and fill_cull(tile_recs,
  // cull_recs, cull_wins) -> bool queue the fill kernels for this launch's frame.  A fill that
  // fails is no error of the frame: the launch runs what it would run without that cache.
  // tk: the launch's TexKey (tk->cull equal to ck), or null: no texel layer for this launch.
  // compact_ok: the launch is eligible for the compact layer (the option, no supersampling, every
  // texel index the records can name below kCompactOutside, a class table that fits).
  // pixel_generation: the world's count of atlas writes for a launch that takes part in the pixel
  // layer (a plain render_band with the option on; n.pixels its band's bytes), or < 0: no pixel
  // layer for this launch -- it neither reads nor fills it, and drops it only with a layer under it.
  template <class Dev>
  TraceCaches begin(const RayKey& rk, const CullKey& ck, const CacheSizes& n, long long other_ray,
                    long long other_hit, long long ray_budget, long long hit_budget, Dev&& dev,
                    const TexKey* tk = nullptr, bool compact_ok = false, long long pixel_generation = -1) {
    const auto free_fn = [&dev](void* p) { return dev.free(p); };
    const auto reserve = [&](CacheBuf& b, long long m) {
      return b.reserve(m, free_fn, [&dev](long long q) { return dev.alloc(q); });
    };
    ray_key = rk;
    cull_key = ck;
    have_tex_key = tk != nullptr;
    if (tk) tex_key = *tk;
    have_pixel_key = tk != nullptr && pixel_generation >= 0;
    if (have_pixel_key) {
      pixel_key.tex = *tk;
      pixel_key.generation = (unsigned long long)pixel_generation;
    }
    TraceCaches d;
    d.decided = true;
    d.ray = ray.decide(rk, RayAction::kRead, n.dirs, dirs.bytes, other_ray, ray_budget);
    if (d.ray == RayAction::kFill) {
      // The tile records are rewritten: what rides on them goes first and takes no room from the
      // directions.  have_prev stays, so this very launch can go on to fill all three.
      for (CacheBuf* b : {&pixels, &cull_recs, &cull_wins, &hit_recs, &texel_recs, &compact_recs})
        b->release(free_fn);
      cull.valid = false;
      hit.valid = false;
      texel.valid = false;
      compact.valid = false;
      pixel.valid = false;
      if (!reserve(dirs, n.dirs) || !reserve(tile_recs, n.tile_recs) ||
          !dev.fill_rays((float*)dirs.ptr, (TileRec*)tile_recs.ptr)) {
        invalidate();  // the buffers may be gone or half written
        d.ray = RayAction::kTrace;
      }
    }
    if (d.ray != RayAction::kTrace) {
      d.dirs = (const float*)dirs.ptr;
      d.tile_recs = (const TileRec*)tile_recs.ptr;
    }
    // The cull cache, on top of the tile records this launch reads (or has just filled).
    d.cull = cull.decide(ck, d.ray, n.cull_recs + n.cull_wins, cull_bytes(), other_ray + dirs.bytes,
                         ray_budget);
    if (d.cull == RayAction::kFill &&
        (!reserve(cull_recs, n.cull_recs) || !reserve(cull_wins, n.cull_wins) ||
         !dev.fill_cull((const TileRec*)tile_recs.ptr, (CullRec*)cull_recs.ptr, cull_wins.ptr))) {
      cull.invalidate();  // the tile records are whole: the launch reads them
      hit.invalidate();
      texel.invalidate();
      compact.invalidate();
      pixel.invalidate();
      d.cull = RayAction::kTrace;
    }
    if (d.cull != RayAction::kTrace) {
      d.cull_recs = (const CullRec*)cull_recs.ptr;
      d.cull_wins = cull_wins.ptr;
    }
    // The hit cache, on top of the cull cache, under the same key and a budget of its own; the
    // launch that marches anyway fills it, so there is only room to find.
    // (a fill rewrites the records the texel layer was made from: that layer's bytes go first and
    // are this chain's to reuse)
    d.hit = hit.decide(ck, d.cull, n.hit_recs, bytes_under_hit_budget(), other_hit, hit_budget);
    if (d.hit == RayAction::kFill) {
      pixels.release(free_fn);
      pixel.valid = false;
      compact_recs.release(free_fn);
      compact.valid = false;
      texel_recs.release(free_fn);
      texel.valid = false;
      if (!reserve(hit_recs, n.hit_recs)) {
        hit.invalidate();  // no memory for it: the launch stays on the cull-cache path
        texel.invalidate();
        compact.invalidate();
        pixel.invalidate();
        d.hit = RayAction::kTrace;
      }
    }
    if (d.hit != RayAction::kTrace) d.hit_recs = (HitRec*)hit_recs.ptr;
    // The texel cache, on top of the hit cache and under its budget.  It has no fill kernel and the
    // _hf kernels do not store it: only a launch that reads the hit layer fills it.
    if (tk) {
      d.texel = texel.decide(*tk, d.hit, n.texel_recs, texel_recs.bytes, other_hit + hit_recs.bytes,
                             hit_budget);
      if (d.texel == RayAction::kFill && d.hit != RayAction::kRead) d.texel = RayAction::kTrace;
      if (d.texel == RayAction::kFill) {
        // (the compact records were made from the ones about to be rewritten: they go first, and
        // the decision above did not count them; the pixels before them)
        pixels.release(free_fn);
        pixel.valid = false;
        compact_recs.release(free_fn);
        compact.valid = false;
        if (!reserve(texel_recs, n.texel_recs)) {
          texel.invalidate();  // no memory for it: the launch reads the hit layer
          compact.invalidate();
          pixel.invalidate();
          d.texel = RayAction::kTrace;
        }
      }
      if (d.texel != RayAction::kTrace) d.texel_recs = (TexelRec*)texel_recs.ptr;
      // The compact layer, on top of the texel layer and under the same budget, after the hit and
      // texel records have theirs.  Only a launch that reads the texel layer fills it.
      d.compact = compact.decide(*tk, d.texel, compact_ok ? n.compact_recs : 0, compact_recs.bytes,
                                 other_hit + hit_recs.bytes + texel_recs.bytes, hit_budget);
      if (d.compact == RayAction::kFill && d.texel != RayAction::kRead) d.compact = RayAction::kTrace;
      if (d.compact == RayAction::kFill) {
        // (the pixels were shaded from the layer under this one: they go first, whatever their
        // launch would have read, and the decision above did not count them)
        pixels.release(free_fn);
        pixel.valid = false;
        if (!reserve(compact_recs, n.compact_recs)) {
          compact.invalidate();  // no memory for it: the launch reads the texel layer
          pixel.invalidate();
          d.compact = RayAction::kTrace;
        }
      }
      if (d.compact != RayAction::kTrace) d.compact_recs = (CompactRec*)compact_recs.ptr;
      // The pixel layer, on top of the compact layer -- of the texel layer where the launch has no
      // compact layer -- and under the same budget, after the chain's other layers have theirs.  Only
      // a launch that reads the layer under it fills it, by a copy of the band it wrote.
      if (have_pixel_key) {
        const RayAction below = d.compact != RayAction::kTrace ? d.compact : d.texel;
        d.pixel = pixel.decide(pixel_key, below, n.pixels, pixels.bytes,
                               other_hit + hit_recs.bytes + texel_recs.bytes + compact_recs.bytes, hit_budget);
        if (d.pixel == RayAction::kFill && below != RayAction::kRead) d.pixel = RayAction::kTrace;
        if (d.pixel == RayAction::kFill && !reserve(pixels, n.pixels)) {
          pixel.invalidate();  // no memory for it: the launch shades from the layer under it
          d.pixel = RayAction::kTrace;
        }
        if (d.pixel != RayAction::kTrace) d.pixels = (uint32_t*)pixels.ptr;
      }
    }
    return d;
  }

  // After the launch begin() decided d for was queued (queued = false: it failed).
  void end(const TraceCaches& d, bool queued, CacheCounters& n) {
    if (!queued) {
      invalidate();
      return;
    }
    const bool ray_filled = d.ray == RayAction::kFill, cull_filled = d.cull == RayAction::kFill;
    ray.commit(ray_key, d.ray, false);
    cull.commit(cull_key, d.cull, ray_filled);
    hit.commit(cull_key, d.hit, ray_filled || cull_filled);
    const bool hit_filled = d.hit == RayAction::kFill;
    if (have_tex_key) {
      texel.commit(tex_key, d.texel, ray_filled || cull_filled || hit_filled);
      compact.commit(tex_key, d.compact,
                     ray_filled || cull_filled || hit_filled || d.texel == RayAction::kFill);
    } else if (ray_filled || cull_filled || hit_filled) {
      texel.valid = false;
      compact.valid = false;
    }
    const bool below_pixel_filled = ray_filled || cull_filled || hit_filled ||
                                    d.texel == RayAction::kFill || d.compact == RayAction::kFill;
    if (have_pixel_key) {
      pixel.commit(pixel_key, d.pixel, below_pixel_filled);
    } else {
      if (below_pixel_filled) pixel.valid = false;
      pixel.have_prev = false;  // a launch without the layer came between two of a key
    }
    n.ray_fills += ray_filled;
    n.ray_cached_frames += d.ray != RayAction::kTrace;
    n.cull_fills += cull_filled;
    n.cull_hits += d.cull == RayAction::kRead;
    n.hit_fills += d.hit == RayAction::kFill;
    n.hit_hits += d.hit == RayAction::kRead;
    n.texel_fills += d.texel == RayAction::kFill;
    n.texel_hits += d.texel == RayAction::kRead;
    n.compact_fills += d.compact == RayAction::kFill;
    n.compact_hits += d.compact == RayAction::kRead;
    n.pixel_fills += d.pixel == RayAction::kFill;
    n.pixel_hits += d.pixel == RayAction::kRead;
  }

  void invalidate() {
    ray.invalidate();
    cull.invalidate();
    invalidate_hit();
  }
  void invalidate_hit() {
    hit.invalidate();
    invalidate_texel();
  }
  void invalidate_texel() {
    texel.invalidate();
    invalidate_compact();
  }
  void invalidate_compact() {
    compact.invalidate();
    pixel.invalidate();
  }
  void invalidate_pixel() { pixel.invalidate(); }

  // Freed by the host once the device has drained (an option lowered, the world going away).
  template <class Free>
  void release_hit(Free&& free_fn) {
    pixels.release(free_fn);
    compact_recs.release(free_fn);
    hit_recs.release(free_fn);
    texel_recs.release(free_fn);
    invalidate_hit();
  }
  template <class Free>
  void release_texel(Free&& free_fn) {
    pixels.release(free_fn);
    compact_recs.release(free_fn);
    texel_recs.release(free_fn);
    invalidate_texel();
  }
  template <class Free>
  void release_compact(Free&& free_fn) {
    pixels.release(free_fn);
    compact_recs.release(free_fn);
    invalidate_compact();
  }
  template <class Free>
  void release_pixel(Free&& free_fn) {
    pixels.release(free_fn);
    pixel.invalidate();
  }
  template <class Free>
  void release_all(Free&& free_fn) {
    for (CacheBuf* b : {&pixels, &dirs, &tile_recs, &cull_recs, &cull_wins, &hit_recs, &texel_recs, &compact_recs})
      b->release(free_fn);
    invalidate();
  }
};

}  // namespace sfrt
