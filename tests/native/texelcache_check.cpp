// texelcache_check.cpp -- the texel cache and its record (csrc/sfrt_raycache.h TexelRec, TexKey,
// the texel layer of ChainCaches) on the host: no HIP.  Every launch goes through
// ChainCaches::begin / end with the launch's TexKey, as sfrt_world.cpp sched_begin calls them:
// the directions decide first, then the cull cache, the hit cache, and on a launch that reads the
// hit cache the texel cache, under the hit cache's budget.  Built and run by
// tests/test_texel_cache_policy.py (g++, with -fsanitize=address,undefined).
#include <cmath>
#include <cstring>
#include <limits>
#include <utility>

#include "chain_harness.h"

using sfrt::TexKey;

static inline bool is4(const TraceCaches& d, RayAction r, RayAction c, RayAction h, RayAction x) {
  return is(d, r, c, h) && d.texel == x;
}

// The frame with what the key does not hold: the atlas the launch reads and its texels.
struct TexFrame : Frame {
  const void* atlas = nullptr;
  unsigned texel_generation = 0;

  TexKey tex_key() const {
    TexKey k;
    k.cull = key();
    k.set_textures(recs.data(), (int)recs.size());
    return k;
  }
};

constexpr long long kHit = 9 * 4 * 64 * 16, kTex = 9 * 4 * 64 * 8;

// One chain on the frames' grid whose launches carry a TexKey (texels = false: SFRT_OPT_TEXEL_CACHE
// 0 -- the launch passes no key and a size of 0).
struct TexChain : Chain {
  using Chain::Chain;
  bool texels = true;

  TraceCaches launch(const TexFrame& f, bool queued = true) {
    const CullKey key = f.key();
    const TexKey tk = f.tex_key();
    const sfrt::CacheSizes n{sfrt::ray_cache_bytes(kTiles, kRays), sfrt::tile_rec_bytes(kTiles),
                             sfrt::cull_rec_bytes(kTiles), sfrt::cull_win_bytes(kTiles, key.n > 64),
                             sfrt::hit_cache_bytes(kTiles, kRays),
                             texels ? sfrt::texel_cache_bytes(kTiles, kRays) : 0};
    const TraceCaches d = caches.begin(key.ray, key, n, others, hit_others, budget, hit_budget, dev,
                                       texels ? &tk : nullptr);
    caches.end(d, queued, stats);
    if (!queued) chain_k = 0;
    else if (!d.reading()) chain_k++;
    // chain_harness.h's post-conditions, and the same one layer up
    EXPECT(!caches.cull.valid || caches.ray.valid);
    EXPECT(!caches.hit.valid || caches.cull.valid);
    EXPECT(!caches.hit.valid || caches.hit.cached.same(caches.cull.cached));
    EXPECT(!caches.texel.valid || caches.hit.valid);
    EXPECT(!caches.texel.valid || caches.texel.cached.cull.same(caches.hit.cached));
    EXPECT(!caches.texel.valid || caches.texel_recs.bytes == sfrt::texel_cache_bytes(kTiles, kRays));
    EXPECT(d.cull == T || d.ray != T);
    EXPECT(d.hit == T || d.cull != T);
    EXPECT(d.texel == T || d.hit == R);  // filled and read only by a launch that reads the hit layer
    EXPECT((d.ray != T) == (d.dirs != nullptr) && (d.ray != T) == (d.tile_recs != nullptr));
    EXPECT((d.cull != T) == (d.cull_recs != nullptr) && (d.cull != T) == (d.cull_wins != nullptr));
    EXPECT((d.hit != T) == (d.hit_recs != nullptr));
    EXPECT((d.texel != T) == (d.texel_recs != nullptr));
    EXPECT(d.texel != R || d.reading());  // a reading launch for the scheduler
    // the hit records stay while the texel layer is valid: a resize needs them at once
    EXPECT(!caches.texel.valid || caches.hit_recs.bytes == sfrt::hit_cache_bytes(kTiles, kRays));
    return d;
  }
};

static void rest_sequence() {
  TexChain c;
  TexFrame f;
  EXPECT(is4(c.launch(f), T, T, T, T));
  EXPECT(is4(c.launch(f), F, F, F, T));  // the _hf march does not store texel records
  EXPECT(c.caches.texel_recs.bytes == 0 && c.stats.texel_fills == 0);
  EXPECT(is4(c.launch(f), R, R, R, F));  // the hit read also stores them
  EXPECT(c.caches.texel_recs.bytes == kTex && c.stats.texel_fills == 1 && c.stats.texel_hits == 0);
  for (int q = 0; q < 3; q++) EXPECT(is4(c.launch(f), R, R, R, R));
  EXPECT(c.stats.texel_fills == 1 && c.stats.texel_hits == 3);
  // a texel read counts as a read of the three layers under it
  EXPECT(c.stats.hit_fills == 1 && c.stats.hit_hits == 4 && c.stats.cull_hits == 4 && c.stats.ray_cached_frames == 5);
  EXPECT(c.chain_k == 2);  // the two marching launches only
  EXPECT(c.caches.hit_bytes() == kHit && c.caches.texel_bytes() == kTex && c.caches.bytes_under_hit_budget() == kHit + kTex);
  EXPECT(sfrt::texel_cache_bytes(32400, 4) == 66355200ll);  // the 4K frame at four pixels per lane
  EXPECT(sfrt::texel_cache_bytes(kTiles, kRays) == kTex);
}

// A change of tex_off or tex_wh: the launch of the change reads the hit layer only, the next fills
// the texel layer, the one after reads it.  Nothing under the texel layer moves.
template <class Change>
static void tex_change(const char* what, Change change) {
  TexChain c;
  TexFrame f;
  for (int q = 0; q < 4; q++) c.launch(f);
  EXPECT(c.caches.texel.valid);
  const void* hit_ptr = c.caches.hit_recs.ptr;
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (!is4(d1, R, R, R, T)) { std::printf("FAIL %s: the launch of the change did not read the hit layer only\n", what); failures++; }
  const TraceCaches d2 = c.launch(f);
  if (!is4(d2, R, R, R, F)) { std::printf("FAIL %s: the second launch did not refill\n", what); failures++; }
  EXPECT(is4(c.launch(f), R, R, R, R));
  EXPECT(c.stats.texel_fills == 2 && c.stats.hit_fills == 1 && c.caches.hit_recs.ptr == hit_ptr);
  EXPECT(c.caches.texel_recs.bytes == kTex);  // the buffer was reused, not added to
}

// A change of a CullKey field goes through the hit layer: miss, hit refill (no texel store), hit read
// with the texel fill, texel read.
template <class Change>
static void cull_change(const char* what, bool view, Change change) {
  TexChain c;
  TexFrame f;
  for (int q = 0; q < 4; q++) c.launch(f);
  EXPECT(c.caches.texel.valid);
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (d1.hit != T || d1.texel != T) { std::printf("FAIL %s: first launch of a new key did not miss\n", what); failures++; }
  EXPECT(view ? d1.ray == T : d1.ray == R);
  const TraceCaches d2 = c.launch(f);
  if (d2.hit != F || d2.texel != T) { std::printf("FAIL %s: second launch did not refill the hit layer alone\n", what); failures++; }
  EXPECT(!c.caches.texel.valid && c.caches.texel_recs.bytes == 0);  // a hit refill drops the texel layer
  EXPECT(is4(c.launch(f), R, R, R, F));
  EXPECT(is4(c.launch(f), R, R, R, R));
  EXPECT(c.stats.texel_fills == 2 && c.stats.hit_fills == 2);
}

static void key_changes() {
  tex_change("tex_off", [](TexFrame& f) { f.recs[3].tex_off = 4096u; });
  tex_change("tex_off of record 0", [](TexFrame& f) { f.recs[0].tex_off += 1u; });
  tex_change("tex_wh width", [](TexFrame& f) { f.recs[2].tex_wh = 64u | (128u << 16); });
  tex_change("tex_wh height", [](TexFrame& f) { f.recs[9].tex_wh = 128u | (32u << 16); });
  tex_change("every record's slot", [](TexFrame& f) {
    for (Rec& r : f.recs) { r.tex_off = 16384u; r.tex_wh = 48u | (20u << 16); }
  });
  cull_change("cam x", false, [](TexFrame& f) { f.cam[0] = std::nextafterf(f.cam[0], 1.0f); });
  cull_change("cam y", false, [](TexFrame& f) { f.cam[1] = std::nextafterf(f.cam[1], 1.0f); });
  cull_change("cam z", false, [](TexFrame& f) { f.cam[2] = std::nextafterf(f.cam[2], 1.0f); });
  cull_change("cull margin", false, [](TexFrame& f) { f.cull_margin *= 2.0f; });
  cull_change("first_l", false, [](TexFrame& f) { f.first_l = 0.5f; });
  cull_change("cull", false, [](TexFrame& f) { f.cull = 0; });
  cull_change("n", false, [](TexFrame& f) { f.recs.pop_back(); });
  cull_change("cx", false, [](TexFrame& f) { f.recs[3].cx += 0.5f; });
  cull_change("cy", false, [](TexFrame& f) { f.recs[3].cy += 0.5f; });
  cull_change("cz", false, [](TexFrame& f) { f.recs[3].cz += 0.5f; });
  cull_change("r", false, [](TexFrame& f) { f.recs[9].r += 0.5f; });
  cull_change("s_pass", false, [](TexFrame& f) { f.recs[0].s_pass += 0.5f; });
  cull_change("order", false, [](TexFrame& f) { std::swap(f.recs[1], f.recs[2]); });
  cull_change("fwd", true, [](TexFrame& f) { f.ray.fwd[0] ^= 1u; });
  cull_change("h_inc", true, [](TexFrame& f) { f.ray.h_inc ^= 1u; });
  cull_change("rows", true, [](TexFrame& f) { f.ray.sub_rows = 12; });
  cull_change("tile key", true, [](TexFrame& f) { f.ray.tile_key ^= 1ll << 56; });
  {  // what the key does not hold keeps the layer: the texels, the atlas pointer, the centre's angle term
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    const void* p = c.caches.texel_recs.ptr;
    int dummy = 0;
    f.texel_generation++;
    f.atlas = &dummy;
    f.recs[2].atan_c = 1.0f;
    EXPECT(is4(c.launch(f), R, R, R, R));
    EXPECT(c.caches.texel_recs.ptr == p && c.stats.texel_fills == 1 && c.stats.texel_hits == 2);
  }
  {  // a texture resized every frame never fills the texel layer; the hit layer keeps serving
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 3; q++) c.launch(f);
    for (unsigned q = 0; q < 6; q++) {
      f.recs[0].tex_wh = (100u + q) | (7u << 16);
      EXPECT(is4(c.launch(f), R, R, R, T));
    }
    EXPECT(c.stats.texel_fills == 1 && c.stats.texel_hits == 0 && c.stats.hit_hits == 7);
  }
  {  // a camera step and its return: the records were not touched, both layers read again
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    TexFrame g = f;
    g.cam[0] += 1.0f;
    EXPECT(is4(c.launch(g), R, T, T, T));
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
  {  // a size that comes back after one other frame likewise: the texel layer was not rewritten
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    TexFrame g = f;
    g.recs[1].tex_wh = 3u | (1u << 16);
    EXPECT(is4(c.launch(g), R, R, R, T));
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
}

static void budgets() {
  {  // exactly enough for both
    TexChain c;
    c.hit_budget = kHit + kTex;
    TexFrame f;
    c.launch(f);
    EXPECT(is4(c.launch(f), F, F, F, T));
    EXPECT(is4(c.launch(f), R, R, R, F));
    EXPECT(is4(c.launch(f), R, R, R, R));
    EXPECT(c.caches.bytes_under_hit_budget() == c.hit_budget);
  }
  {  // one byte short: the hit layer still fills, the chain stays on it
    TexChain c;
    c.hit_budget = kHit + kTex - 1;
    TexFrame f;
    c.launch(f);
    EXPECT(is4(c.launch(f), F, F, F, T));
    for (int q = 0; q < 3; q++) EXPECT(is4(c.launch(f), R, R, R, T));
    EXPECT(c.stats.texel_fills == 0 && c.caches.texel_recs.bytes == 0 && c.stats.hit_hits == 3);
    c.hit_budget = kHit + kTex;  // raised: the next launch stores
    EXPECT(is4(c.launch(f), R, R, R, F));
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
  {  // another chain's bytes count
    TexChain c;
    c.hit_budget = 2 * (kHit + kTex) - 1;
    c.hit_others = kHit + kTex;
    c.others = 100 * kMiB;  // the ray budget's bytes do not
    TexFrame f;
    c.launch(f);
    EXPECT(is4(c.launch(f), F, F, F, T));
    EXPECT(is4(c.launch(f), R, R, R, T));
    c.hit_others = kHit + kTex - 1;
    EXPECT(is4(c.launch(f), R, R, R, F));
  }
  {  // a refill of the hit layer reuses the texel layer's bytes: a budget of exactly both serves a
     // chain whose key changes
    TexChain c;
    c.hit_budget = kHit + kTex;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    f.cam[0] += 1.0f;
    EXPECT(is4(c.launch(f), R, T, T, T));
    EXPECT(is4(c.launch(f), R, F, F, T));
    EXPECT(c.caches.bytes_under_hit_budget() == kHit);
    EXPECT(is4(c.launch(f), R, R, R, F));
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
  {  // the option off (no key, size 0): the layer traces and allocates nothing
    TexChain c;
    c.texels = false;
    TexFrame f;
    for (int q = 0; q < 5; q++) c.launch(f);
    EXPECT(is4(c.launch(f), R, R, R, T));
    EXPECT(c.dev.allocs == 5 && c.stats.texel_fills == 0 && c.stats.texel_hits == 0 && c.stats.hit_hits == 4);
  }
  {  // a key with a size of 0 likewise
    TexChain c;
    TexFrame f;
    const CullKey key = f.key();
    const TexKey tk = f.tex_key();
    const sfrt::CacheSizes n{sfrt::ray_cache_bytes(kTiles, kRays), sfrt::tile_rec_bytes(kTiles),
                             sfrt::cull_rec_bytes(kTiles), sfrt::cull_win_bytes(kTiles, false),
                             sfrt::hit_cache_bytes(kTiles, kRays)};
    EXPECT(n.texel_recs == 0);
    for (int q = 0; q < 5; q++) {
      const TraceCaches d = c.caches.begin(key.ray, key, n, 0, 0, c.budget, c.hit_budget, c.dev, &tk);
      c.caches.end(d, true, c.stats);
      EXPECT(d.texel == T && d.texel_recs == nullptr);
    }
    EXPECT(c.dev.allocs == 5 && c.caches.texel_recs.bytes == 0);
  }
  {  // the option turned off at run time (release_texel) and on again
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    c.caches.release_texel([&c](void* p) { return c.dev.free(p); });
    c.texels = false;
    EXPECT(c.caches.texel_bytes() == 0 && c.caches.hit_bytes() == kHit && c.caches.hit.valid);
    EXPECT(is4(c.launch(f), R, R, R, T));
    c.texels = true;
    EXPECT(is4(c.launch(f), R, R, R, T));  // the first launch of the key as far as the layer has seen
    EXPECT(is4(c.launch(f), R, R, R, F));
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
  {  // release_hit frees both
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    c.caches.release_hit([&c](void* p) { return c.dev.free(p); });
    EXPECT(c.caches.bytes_under_hit_budget() == 0 && !c.caches.hit.valid && !c.caches.texel.valid);
    EXPECT(is4(c.launch(f), R, R, T, T));
    EXPECT(is4(c.launch(f), R, R, F, T));
    EXPECT(is4(c.launch(f), R, R, R, F));
  }
}

static void failures_of_the_device() {
  {  // no memory for the texel records: not an error, the launch reads the hit layer, a later one retries
    TexChain c;
    c.dev.fail_alloc_of = kTex;
    TexFrame f;
    c.launch(f); c.launch(f);
    EXPECT(is4(c.launch(f), R, R, R, T));
    EXPECT(!c.caches.texel.valid && c.caches.texel_recs.bytes == 0 && c.caches.hit.valid);
    c.dev.fail_alloc_of = -1;
    EXPECT(is4(c.launch(f), R, R, R, F));  // the launch itself was committed: its key is the previous one
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
  {  // a failed launch drops all four
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    EXPECT(is4(c.launch(f, false), R, R, R, R));
    EXPECT(!c.caches.texel.valid && !c.caches.hit.valid && !c.caches.cull.valid && !c.caches.ray.valid && c.chain_k == 0);
    EXPECT(is4(c.launch(f), T, T, T, T));
    EXPECT(is4(c.launch(f), F, F, F, T));
    EXPECT(is4(c.launch(f), R, R, R, F));
    EXPECT(is4(c.launch(f), R, R, R, R));
  }
  {  // a failed filling launch too: the half-written records are not trusted
    TexChain c;
    TexFrame f;
    c.launch(f); c.launch(f);
    EXPECT(is4(c.launch(f, false), R, R, R, F));
    EXPECT(!c.caches.texel.valid && !c.caches.hit.valid);
    EXPECT(is4(c.launch(f), T, T, T, T));
  }
  {  // a failed fill of the cull cache drops what is above it
    TexChain c;
    TexFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    f.cam[1] += 1.0f;
    c.launch(f);
    c.dev.fail_fill_cull = true;
    EXPECT(is4(c.launch(f), R, T, T, T));
    EXPECT(!c.caches.texel.valid && !c.caches.hit.valid && !c.caches.cull.valid);
  }
}

static void takeover() {
  // Another stream takes the chain over: the caches never see the stream.
  TexChain c;
  TexFrame f;
  for (int q = 0; q < 4; q++) c.launch(f);
  const void* p = c.caches.texel_recs.ptr;
  EXPECT(is4(c.launch(f), R, R, R, R));  // (the launch of the other stream)
  EXPECT(c.caches.texel_recs.ptr == p && c.caches.texel.valid);
  const int k0 = c.chain_k;
  for (int q = 0; q < 5; q++) c.launch(f);
  EXPECT(c.chain_k == k0);  // reading launches do not advance the tile order
  TexFrame g = f;
  g.cam[2] += 0.25f;
  EXPECT(is4(c.launch(g), R, T, T, T));
  EXPECT(c.chain_k == k0 + 1);
}

static TraceCaches launch_beside(TexChain& c, const TexChain& other, const TexFrame& f) {
  c.others = other.caches.bytes_under_ray_budget();
  c.hit_others = other.caches.bytes_under_hit_budget();
  return c.launch(f);
}

static void two_chains() {
  TexFrame f;
  {  // room for both chains' four layers
    TexChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex);
    for (int q = 0; q < 4; q++) launch_beside(a, b, f);
    for (int q = 0; q < 3; q++) launch_beside(b, a, f);
    EXPECT(is4(launch_beside(b, a, f), R, R, R, R) && is4(launch_beside(a, b, f), R, R, R, R));
    EXPECT(a.caches.bytes_under_hit_budget() + b.caches.bytes_under_hit_budget() == a.hit_budget);
  }
  {  // a byte short: the second chain gets its hit records and stays on them until the first lets go
    TexChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex) - 1;
    for (int q = 0; q < 4; q++) launch_beside(a, b, f);
    launch_beside(b, a, f);
    EXPECT(is4(launch_beside(b, a, f), F, F, F, T));
    EXPECT(is4(launch_beside(b, a, f), R, R, R, T) && is4(launch_beside(b, a, f), R, R, R, T));
    EXPECT(is4(launch_beside(a, b, f), R, R, R, R));  // the first chain is none the worse
    a.caches.release_texel([&a](void* p) { return a.dev.free(p); });
    EXPECT(is4(launch_beside(b, a, f), R, R, R, F));
    EXPECT(is4(launch_beside(b, a, f), R, R, R, R));
    // the first chain finds the room taken
    EXPECT(is4(launch_beside(a, b, f), R, R, R, T) && is4(launch_beside(a, b, f), R, R, R, T));
  }
  {  // the texel records of one chain keep the other's hit records out
    TexChain a, b;
    a.hit_budget = b.hit_budget = 2 * kHit + kTex - 1;
    for (int q = 0; q < 4; q++) launch_beside(a, b, f);
    launch_beside(b, a, f);
    EXPECT(is4(launch_beside(b, a, f), F, F, T, T));
    EXPECT(b.caches.bytes_under_hit_budget() == 0);
  }
}

static uint32_t bits(float v) { return sfrt::ray_key_bits(v); }

static void records() {
  static_assert(sizeof(sfrt::TexelRec) == 8 && alignof(sfrt::TexelRec) == 8, "8 bytes per ray");
  // the sentinel: the largest index an atlas load_texture accepts can hold is below it
  EXPECT(sfrt::texel_pack_tex(12345u, true) == 0xffffffffu && sfrt::texel_outside(0xffffffffu));
  EXPECT(sfrt::texel_pack_tex(0u, false) == 0u && !sfrt::texel_outside(0u));
  EXPECT(sfrt::texel_pack_tex(0xfffffffeu, false) == 0xfffffffeu && !sfrt::texel_outside(0xfffffffeu));
  EXPECT(sfrt::texel_index_fits(0xffffffffull) && !sfrt::texel_index_fits(0x100000000ull));
  // the moving bit rides in the brightness' sign: every non-negative value comes back bit for bit
  const float denorm = std::numeric_limits<float>::denorm_min();
  for (float v : {1.0f, 0.0f, 0.75f, denorm, std::numeric_limits<float>::min(), 3.0f / 7.0f}) {
    for (bool moving : {false, true}) {
      const uint32_t w = sfrt::texel_pack_bright(bits(v), moving);
      EXPECT(sfrt::texel_moving(w) == moving);
      EXPECT(sfrt::texel_bright_bits(w) == bits(v));
      EXPECT((w >> 31) == (moving ? 1u : 0u));
    }
  }
  EXPECT(sfrt::texel_pack_bright(bits(1.0f), true) == 0xbf800000u);
  EXPECT(sfrt::texel_pack_bright(bits(denorm), true) == 0x80000001u);
  // NaNs of both signs: the payload comes back, the sign does not -- and a NaN of either sign
  // becomes the same bytes (shade_rgba's conversion gives 0 for every NaN)
  for (uint32_t nan : {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0xffffffffu}) {
    for (bool moving : {false, true}) {
      const uint32_t w = sfrt::texel_pack_bright(nan, moving);
      EXPECT(sfrt::texel_moving(w) == moving);
      const uint32_t back = sfrt::texel_bright_bits(w);
      EXPECT(back == (nan & 0x7fffffffu));
      float fv;
      std::memcpy(&fv, &back, 4);
      EXPECT(std::isnan(fv));
    }
  }
  // the records are indexed like the hit records; the last one of the largest ordered grid stays
  // inside the buffer
  const long long tiles = (1ll << 28) - 1;
  EXPECT((long long)sfrt::hit_rec_at((int)(tiles - 1), 4, 3, 63) * 8 + 8 == sfrt::texel_cache_bytes(tiles, 4));
}

int main() {
  rest_sequence();
  key_changes();
  budgets();
  failures_of_the_device();
  takeover();
  two_chains();
  records();
  if (failures) {
    std::printf("texelcache_check: %d failures\n", failures);
    return 1;
  }
  std::printf("texelcache_check ok\n");
  return 0;
}
