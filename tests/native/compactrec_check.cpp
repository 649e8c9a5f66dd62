// compactrec_check.cpp -- the compact layer, its record and the brightness classes (csrc/
// sfrt_raycache.h CompactRec, BrightClasses, the compact layer of ChainCaches) on the host: no HIP.
// The class table is held to its definition -- every class one set of 256 results, neighbouring
// classes different, the count an independent recount's -- and every launch of the chain goes
// through ChainCaches::begin / end with the launch's TexKey and eligibility, as sfrt_world.cpp
// sched_begin calls them.  Built and run by tests/test_compact_policy.py (g++, with
// -ffp-contract=off and -fsanitize=address,undefined).
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <utility>

#include "chain_harness.h"

using sfrt::BrightClasses;
using sfrt::TexKey;

static inline bool is5(const TraceCaches& d, RayAction r, RayAction c, RayAction h, RayAction x, RayAction k) {
  return is(d, r, c, h) && d.texel == x && d.compact == k;
}

static uint32_t bits(float v) { return sfrt::ray_key_bits(v); }
static float flt(uint32_t u) { return BrightClasses::from_bits(u); }

// ---- the class table ----

// The 256 results of a brightness, as shade_rgba computes each channel.
static bool same_results(float a, float b, uint32_t* differs_at = nullptr) {
  for (uint32_t c = 0; c < 256; c++) {
    if (sfrt::bright_channel(c, a) != sfrt::bright_channel(c, b)) {
      if (differs_at) *differs_at = c;
      return false;
    }
  }
  return true;
}

static void class_table() {
  const BrightClasses& t = BrightClasses::get();
  const uint32_t n = t.classes();
  EXPECT(t.fits() && n < (1u << 15));
  EXPECT(n == 20229u);  // 20,228 thresholds (the exact Farey count of order 255 is 19,820)
  EXPECT(t.rep[0] == 0u);
  for (uint32_t i = 1; i < n; i++) EXPECT(t.rep[i - 1] < t.rep[i]);
  EXPECT(t.rep[n - 1] == bits(1.0f));  // c * 1.0f == c: the last threshold is k = c
  // every class is one set of results (monotone in b: the two ends suffice) ...
  for (uint32_t i = 0; i < n; i++) {
    const float lo = flt(t.rep[i]);
    const float hi = i + 1 < n ? flt(t.rep[i + 1] - 1u) : 1.0f;
    if (!same_results(lo, hi)) {
      std::printf("FAIL: class %u is not one set of results\n", i);
      failures++;
    }
  }
  // ... and differs from the next for some channel byte
  for (uint32_t i = 0; i + 1 < n; i++) {
    if (same_results(flt(t.rep[i]), flt(t.rep[i + 1]))) {
      std::printf("FAIL: classes %u and %u are one\n", i, i + 1);
      failures++;
    }
  }
  // An independent recount: for every (c, k) the first bit pattern in [+0, 1.0f] whose product
  // reaches k, by bisection over the patterns (the results are monotone in b), not from k / c.
  std::set<uint32_t> jumps;
  for (uint32_t c = 1; c <= 255; c++) {
    for (uint32_t k = 1; k <= c; k++) {
      uint32_t lo = 0, hi = bits(1.0f);  // channel(c, lo) < k <= channel(c, hi)
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sfrt::bright_channel(c, flt(mid)) >= k) hi = mid;
        else lo = mid;
      }
      jumps.insert(hi);
    }
  }
  EXPECT(jumps.size() + 1 == n);
  uint32_t i = 1;
  for (uint32_t j : jumps) {
    if (i < n) EXPECT(t.rep[i] == j);
    i++;
  }
}

static void class_of() {
  const BrightClasses& t = BrightClasses::get();
  const uint32_t n = t.classes();
  EXPECT(t.class_of(0.0f) == 0u);
  EXPECT(t.class_of(std::numeric_limits<float>::denorm_min()) == 0u);
  for (uint32_t nan : {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu})
    EXPECT(t.class_of(flt(nan)) == 0u);
  EXPECT(t.class_of(1.0f) == n - 1);
  for (uint32_t i = 1; i < n; i++) {
    EXPECT(t.class_of(flt(t.rep[i])) == i);
    EXPECT(t.class_of(flt(t.rep[i] - 1u)) == i - 1);
  }
  // the search by itself, as the device calls it, with bit 31 already cleared
  EXPECT(sfrt::bright_class_of(t.rep.data(), n, 0x7f800001u) == 0u);
  EXPECT(sfrt::bright_class_of(t.rep.data(), n, bits(1.0f)) == n - 1);
  EXPECT(sfrt::bright_class_of(t.rep.data(), n, bits(0.5f)) == t.class_of(0.5f));
  // 10^7 random pairs: the class' representative shades every texel to the brightness' own bytes
  std::mt19937 rng(20229u);
  std::uniform_int_distribution<uint32_t> any32;
  std::uniform_int_distribution<uint32_t> unit(0u, bits(1.0f));  // every pattern of [+0, 1]
  std::uniform_real_distribution<float> flat(0.0f, 1.0f);
  long long bad = 0;
  for (int q = 0; q < 10000000; q++) {
    const uint32_t texel = any32(rng);
    float b = (q & 1) ? flat(rng) : flt(unit(rng));
    if (b > 1.0f) b = 1.0f;
    const float rep = flt(t.rep[t.class_of(b)]);
    if (sfrt::bright_shade_rgba(texel, b) != sfrt::bright_shade_rgba(texel, rep)) bad++;
  }
  if (bad) {
    std::printf("FAIL: %lld of 10^7 random pairs shade differently from their class\n", bad);
    failures++;
  }
  // a NaN shades as class 0's +0 does
  const float nan = std::numeric_limits<float>::quiet_NaN();
  EXPECT(sfrt::bright_shade_rgba(0x80fffefdu, nan) == 0x80000000u);
  EXPECT(sfrt::bright_shade_rgba(0x80fffefdu, 0.0f) == 0x80000000u);
  EXPECT(sfrt::bright_shade_rgba(0x12fffe01u, 1.0f) == 0x12fffe01u);
}

static void records() {
  static_assert(sizeof(sfrt::CompactRec) == 4, "one dword per ray");
  const uint32_t last = BrightClasses::get().classes() - 1;
  for (uint32_t tex : {0u, 1u, 16383u, 32063u, 0xfffeu}) {
    for (uint32_t cls : {0u, 1u, last - 1, last, 0x7fffu}) {
      for (bool moving : {false, true}) {
        const uint32_t w = sfrt::compact_pack(tex, false, cls, moving);
        EXPECT(sfrt::compact_tex(w) == tex && !sfrt::compact_outside(w));
        EXPECT(sfrt::compact_class(w) == cls && sfrt::compact_moving(w) == moving);
        const uint32_t o = sfrt::compact_pack(tex, true, cls, moving);
        EXPECT(sfrt::compact_outside(o) && sfrt::compact_tex(o) == 0xffffu);
        EXPECT(sfrt::compact_class(o) == cls && sfrt::compact_moving(o) == moving);
      }
    }
  }
  // the moving bit beside class 0 and beside the last class touches neither
  EXPECT(sfrt::compact_pack(5u, false, 0u, true) == 0x80000005u);
  EXPECT(sfrt::compact_pack(5u, false, 0x7fffu, false) == 0x7fff0005u);
  EXPECT(sfrt::compact_pack(5u, true, 0u, false) == 0x0000ffffu);
  EXPECT(sfrt::compact_index_fits(0xffffull) && !sfrt::compact_index_fits(0x10000ull));
  EXPECT(sfrt::compact_cache_bytes(32400, 4) == 33177600ll);  // the 4K frame at four pixels per lane
  // [tile][lane][r]: a lane's R records are consecutive; the last one ends the buffer
  EXPECT(sfrt::compact_rec_at(0, 4, 1, 0) == 4u && sfrt::compact_rec_at(0, 3, 63, 2) == 191u);
  const long long tiles = (1ll << 28) - 1;
  EXPECT((long long)sfrt::compact_rec_at((int)(tiles - 1), 4, 63, 3) * 4 + 4 == sfrt::compact_cache_bytes(tiles, 4));
}

// ---- the chain ----

struct TexFrame : Frame {
  int ss = 0;  // log2 of the supersampling factor (part of the ray key's tile_key in the world)
  TexKey tex_key() const {
    TexKey k;
    k.cull = key();
    k.set_textures(recs.data(), (int)recs.size());
    return k;
  }
};

constexpr long long kHit = 9 * 4 * 64 * 16, kTex = 9 * 4 * 64 * 8, kCmp = 9 * 4 * 64 * 4;

// One chain on the frames' grid whose launches carry a TexKey and the compact layer's eligibility
// (option = false: SFRT_OPT_COMPACT_TEXELS 0).
struct CompactChain : Chain {
  using Chain::Chain;
  bool option = true;

  TraceCaches launch(const TexFrame& f, bool queued = true) {
    const CullKey key = f.key();
    const TexKey tk = f.tex_key();
    const bool ok = option && sfrt::compact_eligible(f.recs.data(), (int)f.recs.size(), f.ss);
    const sfrt::CacheSizes n{sfrt::ray_cache_bytes(kTiles, kRays), sfrt::tile_rec_bytes(kTiles),
                             sfrt::cull_rec_bytes(kTiles), sfrt::cull_win_bytes(kTiles, key.n > 64),
                             sfrt::hit_cache_bytes(kTiles, kRays), sfrt::texel_cache_bytes(kTiles, kRays),
                             ok ? sfrt::compact_cache_bytes(kTiles, kRays) : 0};
    const TraceCaches d = caches.begin(key.ray, key, n, others, hit_others, budget, hit_budget, dev, &tk, ok);
    caches.end(d, queued, stats);
    if (!queued) chain_k = 0;
    else if (!d.reading()) chain_k++;
    // the layering rules, one layer up from texelcache_check.cpp's
    EXPECT(!caches.texel.valid || caches.hit.valid);
    EXPECT(!caches.compact.valid || caches.texel.valid);
    EXPECT(!caches.compact.valid || caches.compact.cached.same(caches.texel.cached));
    EXPECT(!caches.compact.valid || caches.compact_recs.bytes == kCmp);
    EXPECT(d.texel == T || d.hit == R);
    EXPECT(d.compact == T || d.texel == R);  // filled and read only by a launch that reads the texel layer
    EXPECT((d.texel != T) == (d.texel_recs != nullptr));
    EXPECT((d.compact != T) == (d.compact_recs != nullptr));
    EXPECT(d.compact == T || ok);
    // the 8-byte layer stays while the compact one is valid: a camera step's return needs neither
    // rewritten, a resize falls back on the hit records
    EXPECT(!caches.compact.valid || (caches.texel_recs.bytes == kTex && caches.hit_recs.bytes == kHit));
    EXPECT(caches.bytes_under_hit_budget() == caches.hit_bytes() + caches.texel_bytes() + caches.compact_bytes());
    return d;
  }
  void to_rest(const TexFrame& f) {
    for (int q = 0; q < 5; q++) launch(f);
    EXPECT(caches.compact.valid);
  }
};

static void rest_sequence() {
  CompactChain c;
  TexFrame f;
  EXPECT(is5(c.launch(f), T, T, T, T, T));
  EXPECT(is5(c.launch(f), F, F, F, T, T));
  EXPECT(is5(c.launch(f), R, R, R, F, T));  // the texel fill does not store compact records
  EXPECT(c.caches.compact_bytes() == 0 && c.stats.compact_fills == 0);
  EXPECT(is5(c.launch(f), R, R, R, R, F));
  EXPECT(c.caches.compact_bytes() == kCmp && c.stats.compact_fills == 1 && c.stats.compact_hits == 0);
  for (int q = 0; q < 3; q++) EXPECT(is5(c.launch(f), R, R, R, R, R));
  EXPECT(c.stats.compact_fills == 1 && c.stats.compact_hits == 3);
  // a compact read counts as a read of the four layers under it
  EXPECT(c.stats.texel_fills == 1 && c.stats.texel_hits == 4 && c.stats.hit_hits == 5 &&
         c.stats.cull_hits == 5 && c.stats.ray_cached_frames == 6);
  EXPECT(c.chain_k == 2);
  EXPECT(c.caches.texel_bytes() == kTex && c.caches.bytes_under_hit_budget() == kHit + kTex + kCmp);
}

// A change of tex_off or tex_wh (still eligible): the launch of the change reads the hit layer, the
// next refills the texel layer and drops the compact one, the one after fills it, the next reads.
template <class Change>
static void tex_change(const char* what, Change change) {
  CompactChain c;
  TexFrame f;
  c.to_rest(f);
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (!is5(d1, R, R, R, T, T)) { std::printf("FAIL %s: the launch of the change\n", what); failures++; }
  EXPECT(c.caches.compact_bytes() == kCmp);  // nothing was rewritten yet
  const TraceCaches d2 = c.launch(f);
  if (!is5(d2, R, R, R, F, T)) { std::printf("FAIL %s: the texel refill\n", what); failures++; }
  EXPECT(!c.caches.compact.valid && c.caches.compact_bytes() == 0);  // dropped and freed first
  EXPECT(is5(c.launch(f), R, R, R, R, F));
  EXPECT(is5(c.launch(f), R, R, R, R, R));
  EXPECT(c.stats.compact_fills == 2 && c.stats.texel_fills == 2 && c.stats.hit_fills == 1);
}

template <class Change>
static void cull_change(const char* what, Change change) {
  CompactChain c;
  TexFrame f;
  c.to_rest(f);
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (d1.hit != T || d1.texel != T || d1.compact != T) { std::printf("FAIL %s: no miss\n", what); failures++; }
  const TraceCaches d2 = c.launch(f);
  if (d2.hit != F || d2.texel != T || d2.compact != T) { std::printf("FAIL %s: the hit refill\n", what); failures++; }
  EXPECT(c.caches.bytes_under_hit_budget() == kHit);  // both upper layers freed
  EXPECT(is5(c.launch(f), R, R, R, F, T));
  EXPECT(is5(c.launch(f), R, R, R, R, F));
  EXPECT(is5(c.launch(f), R, R, R, R, R));
  EXPECT(c.stats.compact_fills == 2);
}

static void key_changes() {
  tex_change("tex_off", [](TexFrame& f) { f.recs[3].tex_off = 4096u; });
  tex_change("tex_off of record 0", [](TexFrame& f) { f.recs[0].tex_off += 1u; });
  tex_change("tex_wh width", [](TexFrame& f) { f.recs[2].tex_wh = 64u | (128u << 16); });
  tex_change("tex_wh height", [](TexFrame& f) { f.recs[9].tex_wh = 128u | (32u << 16); });
  cull_change("cam x", [](TexFrame& f) { f.cam[0] = std::nextafterf(f.cam[0], 1.0f); });
  cull_change("cull margin", [](TexFrame& f) { f.cull_margin *= 2.0f; });
  cull_change("first_l", [](TexFrame& f) { f.first_l = 0.5f; });
  cull_change("cull", [](TexFrame& f) { f.cull = 0; });
  cull_change("n", [](TexFrame& f) { f.recs.pop_back(); });
  cull_change("cx", [](TexFrame& f) { f.recs[3].cx += 0.5f; });
  cull_change("r", [](TexFrame& f) { f.recs[9].r += 0.5f; });
  cull_change("s_pass", [](TexFrame& f) { f.recs[0].s_pass += 0.5f; });
  cull_change("fwd", [](TexFrame& f) { f.ray.fwd[0] ^= 1u; });
  cull_change("rows", [](TexFrame& f) { f.ray.sub_rows = 12; });
  cull_change("tile key", [](TexFrame& f) { f.ray.tile_key ^= 1ll << 56; });
  {  // a camera step and its return: nothing was rewritten, all five read again
    CompactChain c;
    TexFrame f;
    c.to_rest(f);
    TexFrame g = f;
    g.cam[0] += 1.0f;
    EXPECT(is5(c.launch(g), R, T, T, T, T));
    EXPECT(is5(c.launch(f), R, R, R, R, R));
  }
  {  // a size that comes back after one other frame likewise
    CompactChain c;
    TexFrame f;
    c.to_rest(f);
    TexFrame g = f;
    g.recs[1].tex_wh = 3u | (1u << 16);
    EXPECT(is5(c.launch(g), R, R, R, T, T));
    EXPECT(is5(c.launch(f), R, R, R, R, R));
  }
}

static void eligibility() {
  {  // a texture that ends at texel 65,535 fills; one texel more never does
    TexFrame f;
    f.recs[0].tex_off = 0u;
    f.recs[0].tex_wh = 65535u | (1u << 16);
    EXPECT(sfrt::compact_texel_end(f.recs.data(), 10) == 65535ull);
    EXPECT(sfrt::compact_eligible(f.recs.data(), 10, 0) && !sfrt::compact_eligible(f.recs.data(), 10, 1));
    CompactChain c;
    c.to_rest(f);
    f.recs[0].tex_wh = 256u | (256u << 16);
    EXPECT(sfrt::compact_texel_end(f.recs.data(), 10) == 65536ull && !sfrt::compact_eligible(f.recs.data(), 10, 0));
    EXPECT(is5(c.launch(f), R, R, R, T, T));
    EXPECT(is5(c.launch(f), R, R, R, F, T));
    for (int q = 0; q < 4; q++) EXPECT(is5(c.launch(f), R, R, R, R, T));
    EXPECT(c.stats.compact_fills == 1 && c.caches.compact_bytes() == 0);
  }
  {  // the offset counts: 16,384 texels at offset 49,152 is one too many; records past n do not
    TexFrame f;
    f.recs[9].tex_off = 49152u;
    EXPECT(sfrt::compact_texel_end(f.recs.data(), 10) == 65536ull);
    EXPECT(sfrt::compact_texel_end(f.recs.data(), 9) == 16384ull);
    f.recs[9].tex_off = 49151u;
    EXPECT(sfrt::compact_eligible(f.recs.data(), 10, 0));
  }
  {  // supersampled: never filled, the chain stays on the texel layer
    CompactChain c;
    TexFrame f;
    f.ss = 1;
    for (int q = 0; q < 4; q++) c.launch(f);
    for (int q = 0; q < 3; q++) EXPECT(is5(c.launch(f), R, R, R, R, T));
    EXPECT(c.stats.compact_fills == 0 && c.caches.compact_bytes() == 0 && c.dev.allocs == 6);
  }
  {  // the option off: likewise; turned off at run time it frees that layer only, and on again it
     // fills on the second launch it sees
    CompactChain c;
    TexFrame f;
    c.option = false;
    for (int q = 0; q < 6; q++) c.launch(f);
    EXPECT(c.stats.compact_fills == 0 && c.dev.allocs == 6);
    c.option = true;
    EXPECT(is5(c.launch(f), R, R, R, R, F));  // the key is the previous launches'
    EXPECT(is5(c.launch(f), R, R, R, R, R));
    c.caches.release_compact([&c](void* p) { return c.dev.free(p); });
    c.option = false;
    EXPECT(c.caches.compact_bytes() == 0 && c.caches.texel.valid && c.caches.texel_bytes() == kTex);
    EXPECT(is5(c.launch(f), R, R, R, R, T));
    c.option = true;
    EXPECT(is5(c.launch(f), R, R, R, R, F));  // the launch with the option off was one of the key
    EXPECT(is5(c.launch(f), R, R, R, R, R));
    c.caches.release_compact([&c](void* p) { return c.dev.free(p); });
    EXPECT(is5(c.launch(f), R, R, R, R, T));  // released: the first launch as far as the layer has seen
    EXPECT(is5(c.launch(f), R, R, R, R, F));
  }
  {  // release_texel and release_hit free it with what it rides on
    CompactChain c;
    TexFrame f;
    c.to_rest(f);
    c.caches.release_texel([&c](void* p) { return c.dev.free(p); });
    EXPECT(c.caches.bytes_under_hit_budget() == kHit && !c.caches.compact.valid);
    EXPECT(is5(c.launch(f), R, R, R, T, T));
    EXPECT(is5(c.launch(f), R, R, R, F, T));
    EXPECT(is5(c.launch(f), R, R, R, R, F));
    c.caches.release_hit([&c](void* p) { return c.dev.free(p); });
    EXPECT(c.caches.bytes_under_hit_budget() == 0 && !c.caches.compact.valid && !c.caches.texel.valid);
  }
}

static void budgets() {
  {  // exactly enough for the three
    CompactChain c;
    c.hit_budget = kHit + kTex + kCmp;
    TexFrame f;
    c.to_rest(f);
    EXPECT(c.caches.bytes_under_hit_budget() == c.hit_budget);
    // a key change: the upper layers' bytes are the chain's to reuse, the hit layer refills
    f.cam[0] += 1.0f;
    EXPECT(is5(c.launch(f), R, T, T, T, T));
    EXPECT(is5(c.launch(f), R, F, F, T, T));
    EXPECT(is5(c.launch(f), R, R, R, F, T));
    EXPECT(is5(c.launch(f), R, R, R, R, F));
    // a texture change: the texel layer refills in a budget with no byte to spare
    f.recs[0].tex_wh = 64u | (64u << 16);
    EXPECT(is5(c.launch(f), R, R, R, T, T));
    EXPECT(is5(c.launch(f), R, R, R, F, T));
    EXPECT(is5(c.launch(f), R, R, R, R, F));
  }
  {  // a byte short: the lower layers fill as without the layer, the chain stays on the texel layer
    CompactChain c;
    c.hit_budget = kHit + kTex + kCmp - 1;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    for (int q = 0; q < 3; q++) EXPECT(is5(c.launch(f), R, R, R, R, T));
    EXPECT(c.stats.compact_fills == 0 && c.caches.compact_bytes() == 0 && c.stats.texel_hits == 4);
    c.hit_budget += 1;  // raised: the next launch stores
    EXPECT(is5(c.launch(f), R, R, R, R, F));
    EXPECT(is5(c.launch(f), R, R, R, R, R));
  }
  {  // exactly the two lower layers: they fill, the compact layer never does
    CompactChain c;
    c.hit_budget = kHit + kTex;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    EXPECT(is5(c.launch(f), R, R, R, R, T));
    EXPECT(c.caches.bytes_under_hit_budget() == kHit + kTex && c.stats.compact_fills == 0);
  }
  {  // another chain's bytes count
    CompactChain c;
    c.hit_budget = 2 * (kHit + kTex + kCmp) - 1;
    c.hit_others = kHit + kTex + kCmp;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    EXPECT(is5(c.launch(f), R, R, R, R, T));
    c.hit_others -= 1;
    EXPECT(is5(c.launch(f), R, R, R, R, F));
  }
}

static void failures_of_the_device() {
  {  // no memory for the compact records: not an error, the launch reads the texel layer, a later one retries
    CompactChain c;
    c.dev.fail_alloc_of = kCmp;
    TexFrame f;
    for (int q = 0; q < 3; q++) c.launch(f);
    EXPECT(is5(c.launch(f), R, R, R, R, T));
    EXPECT(!c.caches.compact.valid && c.caches.compact_bytes() == 0 && c.caches.texel.valid);
    c.dev.fail_alloc_of = -1;
    EXPECT(is5(c.launch(f), R, R, R, R, F));
    EXPECT(is5(c.launch(f), R, R, R, R, R));
  }
  {  // no memory for the texel refill: the compact layer went first and stays gone
    CompactChain c;
    TexFrame f;
    c.to_rest(f);
    f.recs[0].tex_wh = 64u | (64u << 16);
    c.launch(f);
    c.dev.fail_alloc_of = kTex;
    c.caches.texel_recs.release([&c](void* p) { return c.dev.free(p); });  // (so that the refill allocates)
    c.caches.texel.valid = false;
    EXPECT(is5(c.launch(f), R, R, R, T, T));
    EXPECT(!c.caches.compact.valid && !c.caches.texel.valid && c.caches.hit.valid);
    EXPECT(c.caches.bytes_under_hit_budget() == kHit);
  }
  {  // a failed launch drops all five
    CompactChain c;
    TexFrame f;
    c.to_rest(f);
    EXPECT(is5(c.launch(f, false), R, R, R, R, R));
    EXPECT(!c.caches.compact.valid && !c.caches.texel.valid && !c.caches.hit.valid && !c.caches.ray.valid);
    EXPECT(is5(c.launch(f), T, T, T, T, T));
    EXPECT(is5(c.launch(f), F, F, F, T, T));
    EXPECT(is5(c.launch(f), R, R, R, F, T));
    EXPECT(is5(c.launch(f), R, R, R, R, F));
    EXPECT(is5(c.launch(f), R, R, R, R, R));
  }
  {  // a failed filling launch too: the half-written records are not trusted
    CompactChain c;
    TexFrame f;
    for (int q = 0; q < 3; q++) c.launch(f);
    EXPECT(is5(c.launch(f, false), R, R, R, R, F));
    EXPECT(!c.caches.compact.valid && !c.caches.texel.valid);
    EXPECT(is5(c.launch(f), T, T, T, T, T));
  }
  {  // a failed fill of the cull cache drops what is above it
    CompactChain c;
    TexFrame f;
    c.to_rest(f);
    f.cam[1] += 1.0f;
    c.launch(f);
    c.dev.fail_fill_cull = true;
    EXPECT(is5(c.launch(f), R, T, T, T, T));
    EXPECT(!c.caches.compact.valid && !c.caches.texel.valid && !c.caches.hit.valid);
  }
}

static TraceCaches launch_beside(CompactChain& c, const CompactChain& other, const TexFrame& f) {
  c.others = other.caches.bytes_under_ray_budget();
  c.hit_others = other.caches.bytes_under_hit_budget();
  return c.launch(f);
}

static void two_chains() {
  TexFrame f;
  {  // room for both chains' five layers
    CompactChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex + kCmp);
    for (int q = 0; q < 5; q++) launch_beside(a, b, f);
    for (int q = 0; q < 5; q++) launch_beside(b, a, f);
    EXPECT(is5(launch_beside(b, a, f), R, R, R, R, R) && is5(launch_beside(a, b, f), R, R, R, R, R));
    EXPECT(a.caches.bytes_under_hit_budget() + b.caches.bytes_under_hit_budget() == a.hit_budget);
  }
  {  // a byte short: the second chain gets its hit and texel records and stays on them
    CompactChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex + kCmp) - 1;
    for (int q = 0; q < 5; q++) launch_beside(a, b, f);
    for (int q = 0; q < 4; q++) launch_beside(b, a, f);
    EXPECT(is5(launch_beside(b, a, f), R, R, R, R, T));
    EXPECT(is5(launch_beside(a, b, f), R, R, R, R, R));  // the first chain is none the worse
    a.caches.release_compact([&a](void* p) { return a.dev.free(p); });
    EXPECT(is5(launch_beside(b, a, f), R, R, R, R, F));
    EXPECT(is5(launch_beside(b, a, f), R, R, R, R, R));
  }
  {  // The limit sfrt.h states: between chains the compact bytes count like any others.  A budget
     // of two hit and two texel layers, which served two chains before the layer existed: the
     // first chain's compact records keep the second chain's texel layer out until they go.
    CompactChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex);
    for (int q = 0; q < 5; q++) launch_beside(a, b, f);
    EXPECT(a.caches.compact.valid);
    launch_beside(b, a, f);
    EXPECT(is5(launch_beside(b, a, f), F, F, F, T, T));
    EXPECT(is5(launch_beside(b, a, f), R, R, R, T, T));
    a.caches.release_compact([&a](void* p) { return a.dev.free(p); });
    a.option = false;  // SFRT_OPT_COMPACT_TEXELS 0, the remedy
    EXPECT(is5(launch_beside(b, a, f), R, R, R, F, T));
    EXPECT(is5(launch_beside(a, b, f), R, R, R, R, T));
    EXPECT(is5(launch_beside(b, a, f), R, R, R, R, T));  // no room for its own compact records either
  }
}

int main() {
  class_table();
  class_of();
  records();
  rest_sequence();
  key_changes();
  eligibility();
  budgets();
  failures_of_the_device();
  two_chains();
  if (failures) {
    std::printf("compactrec_check: %d failures\n", failures);
    return 1;
  }
  std::printf("compactrec_check ok\n");
  return 0;
}
