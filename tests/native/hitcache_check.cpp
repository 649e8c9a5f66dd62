// hitcache_check.cpp -- the hit cache's policy and record (csrc/sfrt_raycache.h HitRec,
// HitCachePolicy) on the host: no HIP.  A chain is modelled as the world drives it (sfrt_world.cpp
// sched_begin / sched_end): the ray cache decides first, then the cull cache, then the hit cache
// under the cull cache's key and a budget of its own; a fill reserves the chain's CacheBufs
// through counting allocators.  Built and run by tests/test_hit_cache_policy.py (g++, with
// -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "sfrt_raycache.h"

using sfrt::CacheBuf;
using sfrt::CullCachePolicy;
using sfrt::CullKey;
using sfrt::HitCachePolicy;
using sfrt::RayAction;
using sfrt::RayCachePolicy;
using sfrt::RayKey;

static int failures = 0;
#define EXPECT(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

// sfrt_trace.h SphereRec's members (this test needs only the names).
struct Rec {
  float cx, cy, cz, r, s_pass, atan_c;
  uint32_t tex_off, tex_wh;
};

static RayKey base_ray_key() {
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

static std::vector<Rec> base_records(int n) {
  std::vector<Rec> r((size_t)n);
  for (int k = 0; k < n; k++)
    r[(size_t)k] = Rec{0.5f * (float)k, -0.25f * (float)k, 3.0f + (float)k, 1.0f + 0.125f * (float)k,
                      0.75f + (float)k, 0.1f * (float)k, 0u, 128u | (128u << 16)};
  return r;
}

// A launch's frame as far as the cull and the march read it.
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

constexpr long long kMiB = 1ll << 20;
constexpr long long kTiles = 9;
constexpr int kRays = 4;

// What one launch did: the three decisions.
struct Did {
  RayAction ray, cull, hit;
};

// One chain and the world's budgets around it, with counting allocators.
struct Chain {
  RayCachePolicy ray;
  CullCachePolicy cull;
  HitCachePolicy hit;
  CacheBuf ray_dirs, cull_recs, cull_wins, hit_recs;
  long long budget = 512 * kMiB, hit_budget = 512 * kMiB, others = 0, hit_others = 0;
  int allocs = 0, frees = 0, live = 0;
  bool alloc_fails = false, hit_alloc_fails = false;
  int cull_fills = 0, cull_hits = 0, hit_fills = 0, hit_hits = 0, cached_frames = 0;
  int chain_k = 0;  // TileSched::k: launches that advanced the tile order

  ~Chain() {
    for (CacheBuf* b : {&ray_dirs, &cull_recs, &cull_wins, &hit_recs})
      b->release([this](void* p) { return free_fn(p); });
    if (live != 0) {
      std::printf("FAIL: %d buffers leaked\n", live);
      failures++;
    }
  }
  bool free_fn(void* p) {
    std::free(p);
    frees++;
    live--;
    return true;
  }
  void* alloc_fn(long long n, bool fails) {
    if (fails) return nullptr;
    allocs++;
    live++;
    return std::malloc((size_t)n);
  }
  bool reserve(CacheBuf& b, long long n, bool fails = false) {
    return b.reserve(n, [this](void* p) { return free_fn(p); },
                     [this, fails](long long m) { return alloc_fn(m, fails || alloc_fails); });
  }
  long long cull_bytes() const { return cull_recs.bytes + cull_wins.bytes; }
  void invalidate_caches() {  // TileSched::invalidate_caches
    ray.invalidate();
    cull.invalidate();
    hit.invalidate();
  }

  // sched_begin and sched_end of one launch.
  Did launch(const Frame& f, bool queued = true) {
    const RayKey rk = f.ray;
    const long long ray_bytes = sfrt::ray_cache_bytes(kTiles, kRays);
    RayAction ra = ray.decide(rk, ray_bytes, ray_dirs.bytes, others, budget);
    if (ra == RayAction::kFill) {  // release_cull_on: the cull cache and the hit cache on it go first
      for (CacheBuf* b : {&cull_recs, &cull_wins, &hit_recs}) b->release([this](void* p) { return free_fn(p); });
      cull.valid = false;
      hit.valid = false;
    }
    if (ra == RayAction::kFill && !reserve(ray_dirs, ray_bytes)) {
      invalidate_caches();
      ra = RayAction::kTrace;
    }
    const CullKey ck = f.key();
    const bool list = ck.n > 64;
    const long long rb = sfrt::cull_rec_bytes(kTiles), wb = sfrt::cull_win_bytes(kTiles, list);
    RayAction ca = cull.decide(ck, ra, rb + wb, cull_bytes(), others + ray_dirs.bytes, budget);
    if (ca == RayAction::kFill && !(reserve(cull_recs, rb) && reserve(cull_wins, wb))) {
      cull.invalidate();
      hit.invalidate();
      ca = RayAction::kTrace;
    }
    const long long hb = sfrt::hit_cache_bytes(kTiles, kRays);
    RayAction ha = hit.decide(ck, ca, hb, hit_recs.bytes, hit_others, hit_budget);
    if (ha == RayAction::kFill && !reserve(hit_recs, hb, hit_alloc_fails)) {
      hit.invalidate();
      ha = RayAction::kTrace;
    }
    if (!queued) {  // TileSched::end, or the reading launch's own branch: everything goes
      invalidate_caches();
      chain_k = 0;
    } else {
      ray.commit(rk, ra, true);
      cull.commit(ck, ra, ca, true);
      hit.commit(ck, ra, ca, ha, true);
      if (ra != RayAction::kTrace) cached_frames++;
      if (ca == RayAction::kFill) cull_fills++;
      if (ca == RayAction::kRead) cull_hits++;
      if (ha == RayAction::kFill) hit_fills++;
      if (ha == RayAction::kRead) hit_hits++;
      if (ha != RayAction::kRead) chain_k++;  // a reading launch does not advance the chain
    }
    // the invariant of item 5: never valid without a valid cull cache
    EXPECT(!hit.valid || cull.valid);
    EXPECT(!hit.valid || hit.cached.same(cull.cached));
    return Did{ra, ca, ha};
  }
};

static bool is(const Did& d, RayAction r, RayAction c, RayAction h) {
  return d.ray == r && d.cull == c && d.hit == h;
}

constexpr RayAction T = RayAction::kTrace, F = RayAction::kFill, R = RayAction::kRead;

static void first_frames() {
  Chain c;
  Frame f;
  EXPECT(is(c.launch(f), T, T, T));
  EXPECT(c.hit_fills == 0 && c.hit_hits == 0 && c.hit_recs.bytes == 0);
  // the second launch of the key: the directions, the cull and -- the _hf kernel being the _cc one --
  // the march results are all filled by it
  EXPECT(is(c.launch(f), F, F, F));
  EXPECT(c.hit_fills == 1 && c.hit_hits == 0 && c.hit_recs.bytes == sfrt::hit_cache_bytes(kTiles, kRays));
  for (int q = 0; q < 3; q++) EXPECT(is(c.launch(f), R, R, R));
  EXPECT(c.hit_fills == 1 && c.hit_hits == 3 && c.cull_hits == 3 && c.cached_frames == 4);
  EXPECT(c.chain_k == 2);  // the two marching launches only
  EXPECT(sfrt::hit_cache_bytes(32400, 4) == 132710400ll);  // the 4K frame at four pixels per lane
}

// A change of `change` misses, falls back, and the second launch of the new state refills.
template <class Change>
static void key_change(const char* what, bool view, Change change) {
  Chain c;
  Frame f;
  c.launch(f); c.launch(f); c.launch(f);
  EXPECT(c.hit.valid);
  change(f);
  const Did d1 = c.launch(f);
  if (d1.hit != T) { std::printf("FAIL %s: first launch of a new key did not miss\n", what); failures++; }
  EXPECT(view ? d1.ray == T : d1.ray == R);
  const Did d2 = c.launch(f);
  if (d2.hit != F) { std::printf("FAIL %s: second launch of a new key did not refill\n", what); failures++; }
  EXPECT(view ? (d2.ray == F && d2.cull == F) : (d2.ray == R && d2.cull == F));
  EXPECT(is(c.launch(f), R, R, R));
  EXPECT(c.hit_fills == 2);
}

static void key_changes() {
  key_change("cam x", false, [](Frame& f) { f.cam[0] = std::nextafterf(f.cam[0], 1.0f); });
  key_change("cam y", false, [](Frame& f) { f.cam[1] = std::nextafterf(f.cam[1], 1.0f); });
  key_change("cam z", false, [](Frame& f) { f.cam[2] = std::nextafterf(f.cam[2], 1.0f); });
  key_change("cull margin", false, [](Frame& f) { f.cull_margin *= 2.0f; });
  key_change("first_l", false, [](Frame& f) { f.first_l = 0.5f; });
  key_change("cull", false, [](Frame& f) { f.cull = 0; });
  key_change("n", false, [](Frame& f) { f.recs.pop_back(); });
  key_change("cx", false, [](Frame& f) { f.recs[3].cx += 0.5f; });
  key_change("cy", false, [](Frame& f) { f.recs[3].cy += 0.5f; });
  key_change("cz", false, [](Frame& f) { f.recs[3].cz += 0.5f; });
  key_change("r", false, [](Frame& f) { f.recs[9].r += 0.5f; });
  key_change("s_pass", false, [](Frame& f) { f.recs[0].s_pass += 0.5f; });
  key_change("order", false, [](Frame& f) { std::swap(f.recs[1], f.recs[2]); });
  key_change("fwd", true, [](Frame& f) { f.ray.fwd[0] ^= 1u; });
  key_change("h_inc", true, [](Frame& f) { f.ray.h_inc ^= 1u; });
  key_change("rows", true, [](Frame& f) { f.ray.sub_rows = 12; });
  key_change("tile key", true, [](Frame& f) { f.ray.tile_key ^= 1ll << 56; });
  // what the key does not hold keeps hitting: texture slots, the centre's angle term
  Chain c;
  Frame f;
  c.launch(f); c.launch(f);
  f.recs[2].tex_off = 4096u;
  f.recs[2].tex_wh = 64u | (32u << 16);
  f.recs[2].atan_c = 1.0f;
  EXPECT(is(c.launch(f), R, R, R));
  // a key that comes back after one other frame: the records were not touched, the cull cache is
  // valid under the same key, so the launch reads again
  Frame g = f;
  g.cam[0] += 1.0f;
  EXPECT(is(c.launch(g), R, T, T));
  EXPECT(is(c.launch(f), R, R, R));
}

static void refusals() {
  {  // a hit budget too small: the launch stays on the cull-cache path, whose stats are as without
    Chain c;
    c.hit_budget = sfrt::hit_cache_bytes(kTiles, kRays) - 1;
    Frame f;
    c.launch(f);
    EXPECT(is(c.launch(f), F, F, T));
    EXPECT(is(c.launch(f), R, R, T));
    EXPECT(c.hit_fills == 0 && c.hit_hits == 0 && c.hit_recs.bytes == 0 && c.cull_fills == 1 && c.cull_hits == 1);
    c.hit_budget = sfrt::hit_cache_bytes(kTiles, kRays);  // exactly enough: the next launch fills
    EXPECT(is(c.launch(f), R, R, F));
    EXPECT(is(c.launch(f), R, R, R));
  }
  {  // other chains' hit bytes count against the budget, the ray cache's bytes do not
    Chain c;
    c.hit_budget = 2 * sfrt::hit_cache_bytes(kTiles, kRays) - 1;
    c.hit_others = sfrt::hit_cache_bytes(kTiles, kRays);
    c.others = 100 * kMiB;
    Frame f;
    c.launch(f);
    EXPECT(is(c.launch(f), F, F, T));
    c.hit_others = 0;
    EXPECT(is(c.launch(f), R, R, F));
  }
  {  // off: 0
    Chain c;
    c.hit_budget = 0;
    Frame f;
    c.launch(f); c.launch(f);
    EXPECT(is(c.launch(f), R, R, T));
    EXPECT(c.allocs == 3);
  }
  {  // the ray cache's budget at 0 turns everything off
    Chain c;
    c.budget = 0;
    Frame f;
    c.launch(f); c.launch(f);
    EXPECT(is(c.launch(f), T, T, T));
    EXPECT(c.allocs == 0);
  }
  {  // no memory for the records: not an error, the launch stays on the cull cache, a later one retries
    Chain c;
    c.hit_alloc_fails = true;
    Frame f;
    c.launch(f);
    EXPECT(is(c.launch(f), F, F, T));
    EXPECT(!c.hit.valid && c.hit_recs.bytes == 0);
    c.hit_alloc_fails = false;
    EXPECT(is(c.launch(f), R, R, F));  // the launch itself was committed: its key is the previous one
    EXPECT(is(c.launch(f), R, R, R));
  }
}

static void failed_launches() {
  Chain c;
  Frame f;
  c.launch(f); c.launch(f); c.launch(f);
  EXPECT(c.hit.valid);
  EXPECT(is(c.launch(f, false), R, R, R));  // a reading launch that failed: everything goes
  EXPECT(!c.hit.valid && !c.cull.valid && !c.ray.valid && c.chain_k == 0);
  EXPECT(is(c.launch(f), T, T, T));
  EXPECT(is(c.launch(f), F, F, F));
  EXPECT(is(c.launch(f), R, R, R));
  // a failed fill of the directions' buffer drops all three
  Chain d;
  d.launch(f);
  d.alloc_fails = true;
  EXPECT(is(d.launch(f), T, T, T));
  EXPECT(!d.hit.valid && !d.cull.valid && !d.ray.valid);
}

static void takeover() {
  // Another stream takes the chain over: TileSched::begin waits for the device and the chain goes on
  // with every cache as it is -- the policies never see the stream.
  Chain c;
  Frame f;
  c.launch(f); c.launch(f);
  const void* p = c.hit_recs.ptr;
  EXPECT(is(c.launch(f), R, R, R));  // (the launch of the other stream)
  EXPECT(c.hit_recs.ptr == p && c.hit.valid);
  // marching resumes after reading launches as if they had not happened: the chain counted only
  // the marching launches
  const int k0 = c.chain_k;
  for (int q = 0; q < 5; q++) c.launch(f);
  EXPECT(c.chain_k == k0);
  Frame g = f;
  g.cam[2] += 0.25f;
  EXPECT(is(c.launch(g), R, T, T));
  EXPECT(c.chain_k == k0 + 1);
}

static void records() {
  // the packing of drawSphere and the guard bit (sphere_trace.hip hit_store / hit_load use these)
  for (int draw : {0, 1, 63, 64, 1023}) {
    for (bool moving : {false, true}) {
      const uint32_t w = sfrt::hit_pack_draw(draw, moving);
      EXPECT(sfrt::hit_draw(w) == draw);
      EXPECT(sfrt::hit_moving(w) == moving);
      EXPECT((w >> 31) == (moving ? 1u : 0u) && (w & 0x7fffffffu) == (uint32_t)draw);
    }
  }
  // [tile][r][lane]: a ray slot's 64 records are contiguous, a tile's R slots follow each other
  EXPECT(sfrt::hit_rec_at(0, 4, 0, 0) == 0 && sfrt::hit_rec_at(0, 4, 0, 63) == 63);
  EXPECT(sfrt::hit_rec_at(0, 4, 1, 0) == 64 && sfrt::hit_rec_at(1, 4, 0, 0) == 256);
  EXPECT(sfrt::hit_rec_at(5, 3, 2, 7) == (5u * 3u + 2u) * 64u + 7u);
  // the last record of the largest ordered grid stays inside size_t and inside the buffer
  const long long tiles = (1ll << 28) - 1;
  EXPECT((long long)sfrt::hit_rec_at((int)(tiles - 1), 4, 3, 63) * 16 + 16 == sfrt::hit_cache_bytes(tiles, 4));
}

int main() {
  first_frames();
  key_changes();
  refusals();
  failed_launches();
  takeover();
  records();
  if (failures) {
    std::printf("hitcache_check: %d failures\n", failures);
    return 1;
  }
  std::printf("hitcache_check ok\n");
  return 0;
}
