// pixelcache_check.cpp -- the pixel layer of a chain's caches (csrc/sfrt_raycache.h PixelKey, the
// pixel layer of ChainCaches) on the host: no HIP.  Every launch goes through ChainCaches::begin /
// end with the launch's TexKey, eligibility and texel generation, as sfrt_world.cpp sched_begin
// calls them.  Built and run by tests/test_pixel_cache_policy.py (g++, -fsanitize=address,undefined).
#include <cmath>

#include "chain_harness.h"

using sfrt::TexKey;

static inline bool is6(const TraceCaches& d, RayAction r, RayAction c, RayAction h, RayAction x, RayAction k,
                       RayAction p) {
  return is(d, r, c, h) && d.texel == x && d.compact == k && d.pixel == p;
}

struct PixFrame : Frame {
  int ss = 0;           // log2 of the supersampling factor
  long long gen = 1;    // the world's count of atlas writes
  TexKey tex_key() const {
    TexKey k;
    k.cull = key();
    k.set_textures(recs.data(), (int)recs.size());
    return k;
  }
  // the band's output pixels (the frames' 72x20 grid is in samples when ss > 0)
  long long pixel_bytes() const { return sfrt::pixel_cache_bytes(ray.sub_w >> ss, ray.sub_rows >> ss); }
};

constexpr long long kHit = 9 * 4 * 64 * 16, kTex = 9 * 4 * 64 * 8, kCmp = 9 * 4 * 64 * 4, kPix = 72 * 20 * 4;

// One chain on the frames' grid whose launches carry a TexKey, the compact layer's eligibility and
// the pixel layer (option = false: SFRT_OPT_PIXEL_CACHE 0; plain = false: a launch that takes no
// part in the layer, as an aux band's or a pipelined frame's).
struct PixelChain : Chain {
  using Chain::Chain;
  bool option = true, compact_option = true;

  TraceCaches launch(const PixFrame& f, bool queued = true, bool plain = true) {
    const CullKey key = f.key();
    const TexKey tk = f.tex_key();
    const bool ok = compact_option && sfrt::compact_eligible(f.recs.data(), (int)f.recs.size(), f.ss);
    const bool pix = option && plain;
    const sfrt::CacheSizes n{sfrt::ray_cache_bytes(kTiles, kRays), sfrt::tile_rec_bytes(kTiles),
                             sfrt::cull_rec_bytes(kTiles), sfrt::cull_win_bytes(kTiles, key.n > 64),
                             sfrt::hit_cache_bytes(kTiles, kRays), sfrt::texel_cache_bytes(kTiles, kRays),
                             ok ? sfrt::compact_cache_bytes(kTiles, kRays) : 0, pix ? f.pixel_bytes() : 0};
    const void* const pixels_before = caches.pixels.ptr;
    const bool valid_before = caches.pixel.valid;
    const TraceCaches d = caches.begin(key.ray, key, n, others, hit_others, budget, hit_budget, dev, &tk, ok,
                                       pix ? f.gen : -1);
    caches.end(d, queued, stats);
    if (!queued) chain_k = 0;
    else if (!d.reading()) chain_k++;
    // the layering rules, one layer up from compactrec_check.cpp's
    EXPECT(!caches.texel.valid || caches.hit.valid);
    EXPECT(!caches.compact.valid || caches.texel.valid);
    EXPECT(!caches.pixel.valid || caches.texel.valid);
    EXPECT(!caches.pixel.valid || caches.pixel.cached.tex.same(caches.texel.cached));
    EXPECT(!caches.pixel.valid || caches.pixels.bytes > 0);
    EXPECT(d.pixel == T || pix);
    // filled and read only by a launch that reads the topmost layer under it
    EXPECT(d.pixel == T || (d.texel == R && (d.compact == R || d.compact == T)));
    EXPECT(d.pixel != R || (valid_before && d.pixels == pixels_before));
    EXPECT((d.pixel != T) == (d.pixels != nullptr));
    EXPECT((d.texel != T) == (d.texel_recs != nullptr));
    EXPECT((d.compact != T) == (d.compact_recs != nullptr));
    // a lower layer that was filled or refilled left no pixel layer behind, unless this launch made it
    if (d.ray == F || d.cull == F || d.hit == F || d.texel == F || d.compact == F)
      EXPECT(!caches.pixel.valid && caches.pixels.bytes == 0);
    // the lower layers stay while the pixels are valid: a reload falls back on them
    EXPECT(!caches.pixel.valid || (caches.texel_recs.bytes == kTex && caches.hit_recs.bytes == kHit));
    EXPECT(caches.bytes_under_hit_budget() ==
           caches.hit_bytes() + caches.texel_bytes() + caches.compact_bytes() + caches.pixel_bytes());
    return d;
  }
  void to_rest(const PixFrame& f) {
    for (int q = 0; q < 6; q++) launch(f);
    EXPECT(caches.pixel.valid);
  }
  auto free_fn() {
    return [this](void* p) { return dev.free(p); };
  }
};

static void rest_sequence() {
  {
    PixelChain c;
    PixFrame f;
    EXPECT(is6(c.launch(f), T, T, T, T, T, T));
    EXPECT(is6(c.launch(f), F, F, F, T, T, T));
    EXPECT(is6(c.launch(f), R, R, R, F, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));  // the compact fill's band is not copied
    EXPECT(c.caches.pixel_bytes() == 0 && c.stats.pixel_fills == 0);
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    EXPECT(c.caches.pixel_bytes() == kPix && c.stats.pixel_fills == 1 && c.stats.pixel_hits == 0);
    for (int q = 0; q < 3; q++) EXPECT(is6(c.launch(f), R, R, R, R, R, R));
    EXPECT(c.stats.pixel_fills == 1 && c.stats.pixel_hits == 3);
    // a pixel read counts as a read of the five layers under it
    EXPECT(c.stats.compact_fills == 1 && c.stats.compact_hits == 4 && c.stats.texel_hits == 5 &&
           c.stats.hit_hits == 6 && c.stats.cull_hits == 6 && c.stats.ray_cached_frames == 7);
    EXPECT(c.chain_k == 2);  // and links nothing of the tile order
    EXPECT(c.caches.bytes_under_hit_budget() == kHit + kTex + kCmp + kPix);
  }
  {  // a launch not eligible for the compact layer: the fill rides on the texel reader
    PixelChain c;
    PixFrame f;
    f.recs[0].tex_wh = 256u | (256u << 16);
    for (int q = 0; q < 3; q++) c.launch(f);
    EXPECT(is6(c.launch(f), R, R, R, R, T, F));
    EXPECT(is6(c.launch(f), R, R, R, R, T, R));
    EXPECT(c.caches.compact_bytes() == 0 && c.caches.pixel_bytes() == kPix);
  }
  {  // supersampled: the layer holds output pixels
    PixelChain c;
    PixFrame f;
    f.ss = 1;
    EXPECT(f.pixel_bytes() == 36 * 10 * 4);
    for (int q = 0; q < 3; q++) c.launch(f);
    EXPECT(is6(c.launch(f), R, R, R, R, T, F));
    EXPECT(is6(c.launch(f), R, R, R, R, T, R));
    EXPECT(c.caches.pixel_bytes() == 36 * 10 * 4);
  }
  EXPECT(sfrt::pixel_cache_bytes(3840, 2160) == 33177600ll);  // the 4K frame
}

// A reload at the same size: only the generation changes.  The lower layers stay and are read by the
// launch of the change, into the caller's frame; the next launch refills, the one after reads.
static void generation() {
  PixelChain c;
  PixFrame f;
  c.to_rest(f);
  const int allocs = c.dev.allocs;
  f.gen++;
  EXPECT(is6(c.launch(f), R, R, R, R, R, T));
  EXPECT(c.caches.compact.valid && c.caches.texel.valid && c.caches.pixel_bytes() == kPix);
  EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  EXPECT(c.dev.allocs == allocs);  // the buffer is reused
  EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  EXPECT(c.stats.pixel_fills == 2 && c.stats.compact_fills == 1 && c.stats.texel_fills == 1);
  // a reload on every frame never fills, and the frames cost what they cost without the layer
  for (int q = 0; q < 5; q++) {
    f.gen++;
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));
  }
  EXPECT(c.stats.pixel_fills == 2);
  // every other frame: a fill for every reload, never a read
  for (int q = 0; q < 3; q++) {
    f.gen++;
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  }
  // an old generation never comes back (the count only grows), but a key that does is a miss too:
  // the buffer holds the newer pixels
  f.gen--;
  EXPECT(is6(c.launch(f), R, R, R, R, R, T));
}

// A change of tex_off or tex_wh: the texel refill drops the pixels first.
template <class Change>
static void tex_change(const char* what, Change change) {
  PixelChain c;
  PixFrame f;
  c.to_rest(f);
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (!is6(d1, R, R, R, T, T, T)) { std::printf("FAIL %s: the launch of the change\n", what); failures++; }
  EXPECT(c.caches.pixel_bytes() == kPix);  // nothing was rewritten yet
  const TraceCaches d2 = c.launch(f);
  if (!is6(d2, R, R, R, F, T, T)) { std::printf("FAIL %s: the texel refill\n", what); failures++; }
  EXPECT(!c.caches.pixel.valid && c.caches.pixel_bytes() == 0 && c.caches.compact_bytes() == 0);
  EXPECT(is6(c.launch(f), R, R, R, R, F, T));
  EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  EXPECT(c.stats.pixel_fills == 2);
}

template <class Change>
static void cull_change(const char* what, Change change) {
  PixelChain c;
  PixFrame f;
  c.to_rest(f);
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (d1.hit != T || d1.texel != T || d1.compact != T || d1.pixel != T) { std::printf("FAIL %s: no miss\n", what); failures++; }
  const TraceCaches d2 = c.launch(f);
  if (d2.hit != F || d2.pixel != T) { std::printf("FAIL %s: the hit refill\n", what); failures++; }
  EXPECT(c.caches.bytes_under_hit_budget() == kHit);  // the three upper layers freed
  EXPECT(is6(c.launch(f), R, R, R, F, T, T));
  EXPECT(is6(c.launch(f), R, R, R, R, F, T));
  EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  EXPECT(c.stats.pixel_fills == 2);
}

static void key_changes() {
  tex_change("tex_off", [](PixFrame& f) { f.recs[3].tex_off = 4096u; });
  tex_change("tex_off of record 0", [](PixFrame& f) { f.recs[0].tex_off += 1u; });
  tex_change("tex_wh width", [](PixFrame& f) { f.recs[2].tex_wh = 64u | (128u << 16); });
  tex_change("tex_wh height", [](PixFrame& f) { f.recs[9].tex_wh = 128u | (32u << 16); });
  cull_change("cam x", [](PixFrame& f) { f.cam[0] = std::nextafterf(f.cam[0], 1.0f); });
  cull_change("cam y", [](PixFrame& f) { f.cam[1] += 1.0f; });
  cull_change("cam z", [](PixFrame& f) { f.cam[2] += 1.0f; });
  cull_change("cull margin", [](PixFrame& f) { f.cull_margin *= 2.0f; });
  cull_change("first_l", [](PixFrame& f) { f.first_l = 0.5f; });
  cull_change("cull", [](PixFrame& f) { f.cull = 0; });
  cull_change("n", [](PixFrame& f) { f.recs.pop_back(); });
  cull_change("cx", [](PixFrame& f) { f.recs[3].cx += 0.5f; });
  cull_change("cy", [](PixFrame& f) { f.recs[4].cy += 0.5f; });
  cull_change("cz", [](PixFrame& f) { f.recs[5].cz += 0.5f; });
  cull_change("r", [](PixFrame& f) { f.recs[9].r += 0.5f; });
  cull_change("s_pass", [](PixFrame& f) { f.recs[0].s_pass += 0.5f; });
  cull_change("fwd", [](PixFrame& f) { f.ray.fwd[0] ^= 1u; });
  cull_change("right", [](PixFrame& f) { f.ray.right[1] ^= 1u; });
  cull_change("up", [](PixFrame& f) { f.ray.up[2] ^= 1u; });
  cull_change("h_start", [](PixFrame& f) { f.ray.h_start ^= 1u; });
  cull_change("h_inc", [](PixFrame& f) { f.ray.h_inc ^= 1u; });
  cull_change("v_start", [](PixFrame& f) { f.ray.v_start ^= 1u; });
  cull_change("v_inc", [](PixFrame& f) { f.ray.v_inc ^= 1u; });
  // the band and the width (the pixel buffer's own geometry) and the supersampling factor
  cull_change("row0", [](PixFrame& f) { f.ray.sub_row0 = 8; });
  cull_change("rows", [](PixFrame& f) { f.ray.sub_rows = 12; });
  cull_change("width", [](PixFrame& f) { f.ray.sub_w = 71; });
  cull_change("tile key: pixels per lane", [](PixFrame& f) { f.ray.tile_key ^= 1ll << 56; });
  cull_change("tile key: the factor", [](PixFrame& f) { f.ray.tile_key ^= 1ll << 59; });
  {  // a camera step and its return: nothing was rewritten, all six read again
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    PixFrame g = f;
    g.cam[0] += 1.0f;
    EXPECT(is6(c.launch(g), R, T, T, T, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  }
  {  // a size that comes back after one other frame likewise
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    PixFrame g = f;
    g.recs[1].tex_wh = 3u | (1u << 16);
    EXPECT(is6(c.launch(g), R, R, R, T, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  }
  {  // a launch that takes no part (an aux band joins no begin() at all; a pipelined frame does,
     // without the layer): the pixels stay for the next plain launch, but a fill waits for two plain
     // launches in a row
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    EXPECT(is6(c.launch(f, true, false), R, R, R, R, R, T));
    EXPECT(c.caches.pixel.valid && c.caches.pixel_bytes() == kPix);
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
    f.gen++;
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));
    EXPECT(is6(c.launch(f, true, false), R, R, R, R, R, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));  // the first plain launch again
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  }
}

static void lower_refills() {
  {  // the compact layer released and refilled: the pixels go first
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    c.caches.release_compact(c.free_fn());
    EXPECT(!c.caches.pixel.valid && c.caches.pixel_bytes() == 0 && c.caches.texel.valid);
    EXPECT(is6(c.launch(f), R, R, R, R, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  }
  {  // pixels filled over the texel layer, the compact layer turned on later: its fill frees them
    PixelChain c;
    PixFrame f;
    c.compact_option = false;
    for (int q = 0; q < 5; q++) c.launch(f);
    EXPECT(is6(c.launch(f), R, R, R, R, T, R));
    c.compact_option = true;
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));
    EXPECT(!c.caches.pixel.valid && c.caches.pixel_bytes() == 0);
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  }
  {  // release_texel and release_hit free it with what it rides on; release_pixel that layer only
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    c.caches.release_pixel(c.free_fn());
    EXPECT(c.caches.bytes_under_hit_budget() == kHit + kTex + kCmp && c.caches.compact.valid);
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));  // released: the first launch as far as the layer has seen
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    c.caches.release_texel(c.free_fn());
    EXPECT(c.caches.bytes_under_hit_budget() == kHit && !c.caches.pixel.valid);
    c.to_rest(f);
    c.caches.release_hit(c.free_fn());
    EXPECT(c.caches.bytes_under_hit_budget() == 0 && !c.caches.pixel.valid);
  }
  {  // the option off: never filled; turned off at run time it frees that layer only
    PixelChain c;
    PixFrame f;
    c.option = false;
    for (int q = 0; q < 7; q++) c.launch(f);
    EXPECT(c.stats.pixel_fills == 0 && c.dev.allocs == 7 && c.caches.pixel_bytes() == 0);
    c.option = true;
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));  // the launches with the option off were none of the layer's
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
    c.caches.release_pixel(c.free_fn());
    c.option = false;
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));
    EXPECT(c.caches.compact.valid && c.caches.compact_bytes() == kCmp);
  }
}

static void budgets() {
  {  // exactly enough for the four
    PixelChain c;
    c.hit_budget = kHit + kTex + kCmp + kPix;
    PixFrame f;
    c.to_rest(f);
    EXPECT(c.caches.bytes_under_hit_budget() == c.hit_budget);
    // a key change: the upper layers' bytes are the chain's to reuse, every lower layer refills
    f.cam[0] += 1.0f;
    EXPECT(is6(c.launch(f), R, T, T, T, T, T));
    EXPECT(is6(c.launch(f), R, F, F, T, T, T));
    EXPECT(is6(c.launch(f), R, R, R, F, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    // a texture change likewise, in a budget with no byte to spare
    f.recs[0].tex_wh = 64u | (64u << 16);
    EXPECT(is6(c.launch(f), R, R, R, T, T, T));
    EXPECT(is6(c.launch(f), R, R, R, F, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  }
  {  // a byte short: the lower layers fill as without the layer, the chain stays on the compact layer
    PixelChain c;
    c.hit_budget = kHit + kTex + kCmp + kPix - 1;
    PixFrame f;
    for (int q = 0; q < 5; q++) c.launch(f);
    for (int q = 0; q < 3; q++) EXPECT(is6(c.launch(f), R, R, R, R, R, T));
    EXPECT(c.stats.pixel_fills == 0 && c.caches.pixel_bytes() == 0 && c.stats.compact_hits == 4);
    c.hit_budget += 1;  // raised: the next launch is copied
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  }
  {  // the lower layers are never displaced: pixels held over the texel layer in a budget that has
     // room for the compact records only in their place give way to them
    PixelChain c;
    c.hit_budget = kHit + kTex + kCmp;
    c.compact_option = false;
    PixFrame f;
    for (int q = 0; q < 5; q++) c.launch(f);
    EXPECT(is6(c.launch(f), R, R, R, R, T, R));
    EXPECT(c.caches.bytes_under_hit_budget() == kHit + kTex + kPix);
    c.compact_option = true;
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));
    EXPECT(c.caches.bytes_under_hit_budget() == kHit + kTex + kCmp);
    for (int q = 0; q < 3; q++) EXPECT(is6(c.launch(f), R, R, R, R, R, T));  // and no room is left for them
  }
  {  // another chain's bytes count
    PixelChain c;
    c.hit_budget = 2 * (kHit + kTex + kCmp + kPix) - 1;
    c.hit_others = kHit + kTex + kCmp + kPix;
    PixFrame f;
    for (int q = 0; q < 5; q++) c.launch(f);
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));
    c.hit_others -= 1;
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
  }
}

static void failures_of_the_device() {
  {  // no memory for the pixels: not an error, the launch reads the compact layer, a later one retries
    PixelChain c;
    c.dev.fail_alloc_of = kPix;
    PixFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    EXPECT(is6(c.launch(f), R, R, R, R, R, T));
    EXPECT(!c.caches.pixel.valid && c.caches.pixel_bytes() == 0 && c.caches.compact.valid);
    c.dev.fail_alloc_of = -1;
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  }
  {  // a failed launch drops all six
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    EXPECT(is6(c.launch(f, false), R, R, R, R, R, R));
    EXPECT(!c.caches.pixel.valid && !c.caches.compact.valid && !c.caches.texel.valid && !c.caches.hit.valid &&
           !c.caches.ray.valid);
    EXPECT(is6(c.launch(f), T, T, T, T, T, T));
    EXPECT(is6(c.launch(f), F, F, F, T, T, T));
    EXPECT(is6(c.launch(f), R, R, R, F, T, T));
    EXPECT(is6(c.launch(f), R, R, R, R, F, T));
    EXPECT(is6(c.launch(f), R, R, R, R, R, F));
    EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  }
  {  // a failed filling launch (the shading or the copy behind it) too: nothing half-written is trusted
    PixelChain c;
    PixFrame f;
    for (int q = 0; q < 4; q++) c.launch(f);
    EXPECT(is6(c.launch(f, false), R, R, R, R, R, F));
    EXPECT(!c.caches.pixel.valid && !c.caches.compact.valid);
    EXPECT(is6(c.launch(f), T, T, T, T, T, T));
  }
  {  // a failed fill of the cull cache drops what is above it
    PixelChain c;
    PixFrame f;
    c.to_rest(f);
    f.cam[1] += 1.0f;
    c.launch(f);
    c.dev.fail_fill_cull = true;
    EXPECT(is6(c.launch(f), R, T, T, T, T, T));
    EXPECT(!c.caches.pixel.valid && !c.caches.compact.valid && !c.caches.texel.valid && !c.caches.hit.valid);
  }
}

static TraceCaches launch_beside(PixelChain& c, const PixelChain& other, const PixFrame& f) {
  c.others = other.caches.bytes_under_ray_budget();
  c.hit_others = other.caches.bytes_under_hit_budget();
  return c.launch(f);
}

// A takeover: a stream that takes a chain over keeps its caches (the world moves no ChainCaches);
// the launches of the new stream are the same chain's.
static void takeover() {
  PixelChain c;
  PixFrame f;
  c.to_rest(f);
  c.chain_k = 0;  // TileChains::pick handed the chain to another stream: the tile order restarts
  EXPECT(is6(c.launch(f), R, R, R, R, R, R));
  EXPECT(c.chain_k == 0);
}

static void two_chains() {
  PixFrame f;
  {  // room for both chains' six layers
    PixelChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex + kCmp + kPix);
    for (int q = 0; q < 6; q++) launch_beside(a, b, f);
    for (int q = 0; q < 6; q++) launch_beside(b, a, f);
    EXPECT(is6(launch_beside(b, a, f), R, R, R, R, R, R) && is6(launch_beside(a, b, f), R, R, R, R, R, R));
    EXPECT(a.caches.bytes_under_hit_budget() + b.caches.bytes_under_hit_budget() == a.hit_budget);
  }
  {  // The limit sfrt.h states.  Two 4K chains at the default 512 MB: each chain's six layers are
     // 132.7 + 66.4 + 33.2 + 33.2 = 265.4 MB, so both chains' lower layers and one chain's pixels
     // fit and the second chain's pixels do not ...
    const long long hit = sfrt::hit_cache_bytes(32400, 4), tex = sfrt::texel_cache_bytes(32400, 4),
                    cmp = sfrt::compact_cache_bytes(32400, 4), pix = sfrt::pixel_cache_bytes(3840, 2160);
    const long long chain = hit + tex + cmp + pix, budget = 512 * 1000000ll;
    EXPECT(chain == 265420800ll && 2 * chain > budget && 2 * chain - pix <= budget);
    // ... and on the frames' grid a budget in the same position, a byte short of both chains' six:
    // the second chain stays on its compact layer, and the first chain is none the worse
    PixelChain a, b;
    a.hit_budget = b.hit_budget = 2 * (kHit + kTex + kCmp + kPix) - 1;
    for (int q = 0; q < 6; q++) launch_beside(a, b, f);
    for (int q = 0; q < 5; q++) launch_beside(b, a, f);
    EXPECT(is6(launch_beside(b, a, f), R, R, R, R, R, T));
    EXPECT(is6(launch_beside(b, a, f), R, R, R, R, R, T));
    EXPECT(is6(launch_beside(a, b, f), R, R, R, R, R, R));
    EXPECT(b.caches.pixel_bytes() == 0 && b.caches.compact.valid && a.caches.pixel_bytes() == kPix);
    a.caches.release_pixel(a.free_fn());
    EXPECT(is6(launch_beside(b, a, f), R, R, R, R, R, F));
    EXPECT(is6(launch_beside(b, a, f), R, R, R, R, R, R));
    EXPECT(is6(launch_beside(a, b, f), R, R, R, R, R, T));  // now the first chain's do not fit
    EXPECT(is6(launch_beside(a, b, f), R, R, R, R, R, T));
  }
}

int main() {
  rest_sequence();
  generation();
  key_changes();
  lower_refills();
  budgets();
  failures_of_the_device();
  takeover();
  two_chains();
  if (failures) {
    std::printf("pixelcache_check: %d failures\n", failures);
    return 1;
  }
  std::printf("pixelcache_check ok\n");
  return 0;
}
