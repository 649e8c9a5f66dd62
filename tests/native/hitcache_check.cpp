// hitcache_check.cpp -- the hit cache and its record (csrc/sfrt_raycache.h HitRec, the hit layer
// of ChainCaches) on the host: no HIP.  Every launch goes through ChainCaches::begin / end
// (chain_harness.h): the directions decide first, then the cull cache, then the hit cache under the
// cull cache's key and a budget of its own.  Built and run by tests/test_hit_cache_policy.py (g++,
// with -fsanitize=address,undefined).
#include <cmath>
#include <cstring>
#include <utility>

#include "chain_harness.h"

// One chain on the frames' grid.
struct HitChain : Chain {
  using Chain::Chain;
  TraceCaches launch(const Frame& f, bool queued = true) { return Chain::launch(f.key(), kTiles, kRays, queued); }
};

static void first_frames() {
  HitChain c;
  Frame f;
  EXPECT(is(c.launch(f), T, T, T));
  EXPECT(c.stats.hit_fills == 0 && c.stats.hit_hits == 0 && c.caches.hit_recs.bytes == 0);
  // the second launch of the key: the directions, the cull and -- the _hf kernel being the _cc one --
  // the march results are all filled by it
  EXPECT(is(c.launch(f), F, F, F));
  EXPECT(c.stats.hit_fills == 1 && c.stats.hit_hits == 0 && c.caches.hit_recs.bytes == sfrt::hit_cache_bytes(kTiles, kRays));
  for (int q = 0; q < 3; q++) EXPECT(is(c.launch(f), R, R, R));
  EXPECT(c.stats.hit_fills == 1 && c.stats.hit_hits == 3 && c.stats.cull_hits == 3 && c.stats.ray_cached_frames == 4);
  EXPECT(c.chain_k == 2);  // the two marching launches only
  EXPECT(sfrt::hit_cache_bytes(32400, 4) == 132710400ll);  // the 4K frame at four pixels per lane
}

// A change of `change` misses, falls back, and the second launch of the new state refills.
template <class Change>
static void key_change(const char* what, bool view, Change change) {
  HitChain c;
  Frame f;
  c.launch(f); c.launch(f); c.launch(f);
  EXPECT(c.caches.hit.valid);
  change(f);
  const TraceCaches d1 = c.launch(f);
  if (d1.hit != T) { std::printf("FAIL %s: first launch of a new key did not miss\n", what); failures++; }
  EXPECT(view ? d1.ray == T : d1.ray == R);
  const TraceCaches d2 = c.launch(f);
  if (d2.hit != F) { std::printf("FAIL %s: second launch of a new key did not refill\n", what); failures++; }
  EXPECT(view ? (d2.ray == F && d2.cull == F) : (d2.ray == R && d2.cull == F));
  EXPECT(is(c.launch(f), R, R, R));
  EXPECT(c.stats.hit_fills == 2);
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
  HitChain c;
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
    HitChain c;
    c.hit_budget = sfrt::hit_cache_bytes(kTiles, kRays) - 1;
    Frame f;
    c.launch(f);
    EXPECT(is(c.launch(f), F, F, T));
    EXPECT(is(c.launch(f), R, R, T));
    EXPECT(c.stats.hit_fills == 0 && c.stats.hit_hits == 0 && c.caches.hit_recs.bytes == 0 && c.stats.cull_fills == 1 && c.stats.cull_hits == 1);
    c.hit_budget = sfrt::hit_cache_bytes(kTiles, kRays);  // exactly enough: the next launch fills
    EXPECT(is(c.launch(f), R, R, F));
    EXPECT(is(c.launch(f), R, R, R));
  }
  {  // other chains' hit bytes count against the budget, the ray cache's bytes do not
    HitChain c;
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
    HitChain c;
    c.hit_budget = 0;
    Frame f;
    c.launch(f); c.launch(f);
    EXPECT(is(c.launch(f), R, R, T));
    EXPECT(c.dev.allocs == 4);
  }
  {  // the ray cache's budget at 0 turns everything off
    HitChain c;
    c.budget = 0;
    Frame f;
    c.launch(f); c.launch(f);
    EXPECT(is(c.launch(f), T, T, T));
    EXPECT(c.dev.allocs == 0);
  }
  {  // no memory for the records: not an error, the launch stays on the cull cache, a later one retries
    HitChain c;
    c.dev.fail_alloc_of = sfrt::hit_cache_bytes(kTiles, kRays);
    Frame f;
    c.launch(f);
    EXPECT(is(c.launch(f), F, F, T));
    EXPECT(!c.caches.hit.valid && c.caches.hit_recs.bytes == 0);
    c.dev.fail_alloc_of = -1;
    EXPECT(is(c.launch(f), R, R, F));  // the launch itself was committed: its key is the previous one
    EXPECT(is(c.launch(f), R, R, R));
  }
}

static void failed_launches() {
  HitChain c;
  Frame f;
  c.launch(f); c.launch(f); c.launch(f);
  EXPECT(c.caches.hit.valid);
  EXPECT(is(c.launch(f, false), R, R, R));  // a reading launch that failed: everything goes
  EXPECT(!c.caches.hit.valid && !c.caches.cull.valid && !c.caches.ray.valid && c.chain_k == 0);
  EXPECT(is(c.launch(f), T, T, T));
  EXPECT(is(c.launch(f), F, F, F));
  EXPECT(is(c.launch(f), R, R, R));
  // a failed fill of the directions' buffer drops all three
  HitChain d;
  d.launch(f);
  d.dev.fail_alloc = true;
  EXPECT(is(d.launch(f), T, T, T));
  EXPECT(!d.caches.hit.valid && !d.caches.cull.valid && !d.caches.ray.valid);
}

static void takeover() {
  // Another stream takes the chain over: TileSched::begin waits for the device and the chain goes on
  // with every cache as it is -- the caches never see the stream.
  HitChain c;
  Frame f;
  c.launch(f); c.launch(f);
  const void* p = c.caches.hit_recs.ptr;
  EXPECT(is(c.launch(f), R, R, R));  // (the launch of the other stream)
  EXPECT(c.caches.hit_recs.ptr == p && c.caches.hit.valid);
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

// Two chains of one world: each launch is told what the other chain holds, as sched_begin sums it.
static TraceCaches launch_beside(HitChain& c, const HitChain& other, const Frame& f) {
  c.others = other.caches.bytes_under_ray_budget();
  c.hit_others = other.caches.hit_bytes();
  return c.launch(f);
}

static void shared_budgets() {
  const long long ray = sfrt::ray_cache_bytes(kTiles, kRays);
  const long long cull = sfrt::cull_rec_bytes(kTiles) + sfrt::cull_win_bytes(kTiles, false);
  const long long hit = sfrt::hit_cache_bytes(kTiles, kRays);
  Frame f;
  {  // one ray budget: the second chain's fill is refused while the first holds its bytes
    HitChain a, b;
    a.budget = b.budget = 2 * ray + cull - 1;
    launch_beside(a, b, f);
    EXPECT(is(launch_beside(a, b, f), F, F, F));
    EXPECT(a.caches.bytes_under_ray_budget() == ray + cull && a.caches.hit_bytes() == hit);
    EXPECT(a.caches.tile_rec_bytes() == sfrt::tile_rec_bytes(kTiles));  // held, and counted nowhere
    launch_beside(b, a, f);
    EXPECT(is(launch_beside(b, a, f), T, T, T));
    EXPECT(b.dev.allocs == 0);
    EXPECT(is(launch_beside(a, b, f), R, R, R));  // the first chain is none the worse
    a.release();  // (an option lowered, say)
    EXPECT(is(launch_beside(b, a, f), F, F, F));
    EXPECT(is(launch_beside(b, a, f), R, R, R));
  }
  {  // room for the second chain's directions but not for its cull cache
    HitChain a, b;
    a.budget = b.budget = 2 * ray + 2 * cull - 1;
    launch_beside(a, b, f); launch_beside(a, b, f);
    launch_beside(b, a, f);
    EXPECT(is(launch_beside(b, a, f), F, T, T));
    EXPECT(b.caches.bytes_under_ray_budget() == ray);
  }
  {  // both budgets exactly twice one chain's figures: both chains fill everything -- the tile
     // records the two hold are never counted
    HitChain a, b;
    a.budget = b.budget = 2 * (ray + cull);
    a.hit_budget = b.hit_budget = 2 * hit;
    launch_beside(a, b, f); launch_beside(a, b, f);
    launch_beside(b, a, f);
    EXPECT(is(launch_beside(b, a, f), F, F, F));
    EXPECT(a.caches.tile_rec_bytes() + b.caches.tile_rec_bytes() == 2 * sfrt::tile_rec_bytes(kTiles));
    EXPECT(is(launch_beside(a, b, f), R, R, R) && is(launch_beside(b, a, f), R, R, R));
  }
  {  // one hit budget, a byte short of two chains: the second stays on the cull cache until the
     // first lets its records go
    HitChain a, b;
    a.hit_budget = b.hit_budget = 2 * hit - 1;
    launch_beside(a, b, f); launch_beside(a, b, f);
    launch_beside(b, a, f);
    EXPECT(is(launch_beside(b, a, f), F, F, T));
    EXPECT(is(launch_beside(b, a, f), R, R, T) && b.caches.hit_bytes() == 0);
    a.caches.release_hit([&a](void* p) { return a.dev.free(p); });
    EXPECT(a.caches.hit_bytes() == 0 && a.caches.bytes_under_ray_budget() == ray + cull);
    EXPECT(is(launch_beside(b, a, f), R, R, F));
    EXPECT(is(launch_beside(b, a, f), R, R, R));
    // the first chain, its records released, starts over and finds the room taken
    EXPECT(is(launch_beside(a, b, f), R, R, T) && is(launch_beside(a, b, f), R, R, T));
  }
}

// A launch that takes no part (an aux band: sched_begin calls neither begin nor end for it) between
// two reading launches leaves the state and the counters as they were.
static void bystander() {
  HitChain c;
  Frame f;
  c.launch(f); c.launch(f);
  EXPECT(is(c.launch(f), R, R, R));
  const sfrt::CacheCounters n0 = c.stats;
  const sfrt::ChainCaches s0 = c.caches;
  const int allocs0 = c.dev.allocs, k0 = c.chain_k;
  // (the aux launch: nothing of the chain's caches is called)
  EXPECT(std::memcmp(&n0, &c.stats, sizeof n0) == 0 && c.dev.allocs == allocs0 && c.chain_k == k0);
  EXPECT(c.caches.ray.valid && c.caches.cull.valid && c.caches.hit.valid && c.caches.hit.have_prev);
  EXPECT(c.caches.hit_recs.ptr == s0.hit_recs.ptr && c.caches.hit.cached.same(s0.hit.cached));
  EXPECT(is(c.launch(f), R, R, R));
  EXPECT(c.stats.hit_hits == n0.hit_hits + 1 && c.stats.hit_fills == 1 && c.stats.cull_hits == n0.cull_hits + 1 &&
         c.stats.ray_cached_frames == n0.ray_cached_frames + 1);
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
  shared_budgets();
  bystander();
  records();
  if (failures) {
    std::printf("hitcache_check: %d failures\n", failures);
    return 1;
  }
  std::printf("hitcache_check ok\n");
  return 0;
}
