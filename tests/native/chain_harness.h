// chain_harness.h -- what the host checks of a chain's caches share (tilerec_check.cpp,
// cullcache_check.cpp, hitcache_check.cpp): EXPECT, a counting host stand-in for the device, a
// launch's frame as far as the keys hold it, and one launch through the code that ships --
// sfrt_raycache.h ChainCaches::begin / end -- with the layering rules as post-conditions of every
// launch of every scenario.  No HIP.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sfrt_raycache.h"

using sfrt::CullKey;
using sfrt::RayAction;
using sfrt::RayKey;
using sfrt::TraceCaches;

static int failures = 0;
#define EXPECT(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

constexpr long long kMiB = 1ll << 20;
constexpr RayAction T = RayAction::kTrace, F = RayAction::kFill, R = RayAction::kRead;

// The device interface of ChainCaches::begin on the host: every live allocation is a real one
// (the address sanitizer then sees a double free or a leak), counted, and each call can be made
// to fail.
struct Device {
  int allocs = 0, frees = 0, live = 0;
  bool fail_alloc = false, fail_free = false, fail_fill_rays = false, fail_fill_cull = false;
  long long fail_alloc_of = -1;  // an allocation of exactly this many bytes fails

  bool free(void* p) {
    if (fail_free) return false;
    std::free(p);
    frees++;
    live--;
    return true;
  }
  void* alloc(long long n) {
    if (fail_alloc || n == fail_alloc_of) return nullptr;
    allocs++;
    live++;
    return std::malloc((size_t)n);
  }
  bool fill_rays(float* dirs, sfrt::TileRec* tile_recs) { return dirs && tile_recs && !fail_fill_rays; }
  bool fill_cull(const sfrt::TileRec* tile_recs, sfrt::CullRec* cull_recs, void* cull_wins) {
    return tile_recs && cull_recs && cull_wins && !fail_fill_cull;
  }
};

static inline bool is(const TraceCaches& d, RayAction r, RayAction c, RayAction h) {
  return d.ray == r && d.cull == c && d.hit == h;
}

// One chain and the world's two budgets around it.
struct Chain {
  Device own;
  Device& dev;  // its own, or one it shares with other chains
  sfrt::ChainCaches caches;
  sfrt::CacheCounters stats;
  long long budget = 512 * kMiB, hit_budget = 512 * kMiB;  // SFRT_OPT_RAY_CACHE_MB, _HIT_CACHE_MB
  long long others = 0, hit_others = 0;                    // what the other chains hold under them
  int chain_k = 0;  // TileSched::k as the world moves it: launches that advanced the tile order

  Chain() : dev(own) {}
  explicit Chain(Device& shared) : dev(shared) {}
  Chain(const Chain&) = delete;
  ~Chain() {
    release();
    if (own.live != 0) {
      std::printf("FAIL: %d buffers leaked\n", own.live);
      failures++;
    }
  }
  void release() {
    caches.release_all([this](void* p) { return dev.free(p); });
  }

  // sched_begin and sched_end of one launch that takes part, on a grid of `tiles` tiles at `rays`
  // pixels per lane.  queued = false: the launch failed.
  TraceCaches launch(const CullKey& key, long long tiles, int rays, bool queued = true) {
    const sfrt::CacheSizes n{sfrt::ray_cache_bytes(tiles, rays), sfrt::tile_rec_bytes(tiles),
                             sfrt::cull_rec_bytes(tiles), sfrt::cull_win_bytes(tiles, key.n > 64),
                             sfrt::hit_cache_bytes(tiles, rays)};
    const TraceCaches d = caches.begin(key.ray, key, n, others, hit_others, budget, hit_budget, dev);
    caches.end(d, queued, stats);
    if (!queued) chain_k = 0;         // TileSched::reset
    else if (!d.reading()) chain_k++;  // a reading launch does not advance the chain
    // an upper cache is never valid, read or filled without the one under it
    EXPECT(!caches.cull.valid || caches.ray.valid);
    EXPECT(!caches.hit.valid || caches.cull.valid);
    EXPECT(!caches.hit.valid || caches.hit.cached.same(caches.cull.cached));
    EXPECT(d.cull == T || d.ray != T);
    EXPECT(d.hit == T || d.cull != T);
    // the launch gets a layer's buffers exactly when it reads or fills that layer
    EXPECT((d.ray != T) == (d.dirs != nullptr) && (d.ray != T) == (d.tile_recs != nullptr));
    EXPECT((d.cull != T) == (d.cull_recs != nullptr) && (d.cull != T) == (d.cull_wins != nullptr));
    EXPECT((d.hit != T) == (d.hit_recs != nullptr));
    return d;
  }
};

// sfrt_trace.h SphereRec's members, so that the key's field list is checked against the record
// the kernels read (the header itself needs no HIP, but these tests need only the names).
struct Rec {
  float cx, cy, cz, r, s_pass, atan_c;
  uint32_t tex_off, tex_wh;
};

static inline RayKey base_ray_key() {
  RayKey k{};
  const float fwd[3] = {0.0f, 0.0f, 1.0f}, right[3] = {1.0f, 0.0f, 0.0f}, up[3] = {0.0f, -1.0f, 0.0f};
  for (int q = 0; q < 3; q++) {
    k.fwd[q] = sfrt::ray_key_bits(fwd[q]);
    k.right[q] = sfrt::ray_key_bits(right[q]);
    k.up[q] = sfrt::ray_key_bits(up[q]);
  }
  k.h_start = sfrt::ray_key_bits(-1.3f);
  k.h_inc = sfrt::ray_key_bits(0.01f);
  k.v_start = sfrt::ray_key_bits(-0.8f);
  k.v_inc = sfrt::ray_key_bits(0.02f);
  k.xstart = 0; k.xadd = 1; k.ystart = 0; k.yadd = 1;
  k.sub_w = 72; k.sub_row0 = 0; k.sub_rows = 20;
  k.tile_key = (1ll << 62) | (4ll << 56) | (3ll << 28) | 3;
  return k;
}

static inline std::vector<Rec> base_records(int n) {
  std::vector<Rec> r((size_t)n);
  for (int k = 0; k < n; k++)
    r[(size_t)k] = Rec{0.5f * (float)k, -0.25f * (float)k, 3.0f + (float)k, 1.0f + 0.125f * (float)k,
                      0.75f + (float)k, 0.1f * (float)k, 0u, 128u | (128u << 16)};
  return r;
}

// A launch's frame as far as the cull and the march read it: 72x20 at four pixels per lane.
constexpr long long kTiles = 9;
constexpr int kRays = 4;
struct Frame {
  RayKey ray = base_ray_key();
  float cam[3] = {0.25f, -0.5f, 0.125f};
  float cull_margin = 0.0123f, first_l = 0.75f;
  int cull = 1;
  std::vector<Rec> recs = base_records(10);

  CullKey key() const {
    CullKey k;
    k.ray = ray;
    for (int q = 0; q < 3; q++) k.cam[q] = sfrt::ray_key_bits(cam[q]);
    k.cull_margin = sfrt::ray_key_bits(cull_margin);
    k.first_l = sfrt::ray_key_bits(first_l);
    k.cull = cull;
    k.set_records(recs.data(), (int)recs.size());
    return k;
  }
};
