// cullcache_check.cpp -- the cull cache (csrc/sfrt_raycache.h CullKey, the cull layer of
// ChainCaches) on the host: no HIP.  Every launch goes through ChainCaches::begin / end
// (chain_harness.h) with the hit cache off -- its budget 0, as in a diagnostic build -- so the
// chain's allocations are the directions, the tile records and the cull cache's two buffers.
// Built and run by tests/test_cull_cache_policy.py (g++, with -fsanitize=address,undefined).
#include <cstring>
#include <utility>

#include "chain_harness.h"

using CullLayer = sfrt::CacheLayer<CullKey>;

// One chain without a hit cache; a launch returns the cull cache's action.
struct CullChain : Chain {
  RayAction last_ray = T;
  CullChain() { hit_budget = 0; }
  RayAction launch(const Frame& f, bool queued = true) {
    const TraceCaches d = Chain::launch(f.key(), kTiles, kRays, queued);
    EXPECT(d.hit == T && caches.hit_bytes() == 0);
    last_ray = d.ray;
    return d.cull;
  }
};

int main() {
  const Frame f;
  EXPECT(sizeof(sfrt::CullRec) + 64 * sizeof(sfrt::CullWin) == 528);
  EXPECT(sfrt::cull_rec_bytes(32400) + sfrt::cull_win_bytes(32400, false) == 32400ll * 528);
  EXPECT(sfrt::cull_win_bytes(3, true) == 3 * 64 * 12);
  {  // fill on the second identical key (with the ray cache's fill), read on the third
    CullChain c;
    EXPECT(c.launch(f) == RayAction::kTrace && c.last_ray == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill && c.last_ray == RayAction::kFill);
    EXPECT(c.stats.cull_fills == 1 && c.stats.cull_hits == 0 && c.dev.allocs == 4);
    EXPECT(c.launch(f) == RayAction::kRead && c.last_ray == RayAction::kRead);
    EXPECT(c.launch(f) == RayAction::kRead);
    EXPECT(c.stats.cull_fills == 1 && c.stats.cull_hits == 2 && c.dev.allocs == 4 && c.dev.frees == 0);
  }
  {  // each input of the cull, changed alone: today's path, the ray cache still read, a refill on
     // the second launch of the new key into the same buffers, the old key's bits gone
    std::vector<Frame> changed;
    auto with = [&](auto&& change) {
      Frame g = f;
      change(g);
      changed.push_back(g);
    };
    for (int q = 0; q < 3; q++) with([&](Frame& g) { g.cam[q] += 0.5f; });
    with([](Frame& g) { g.cull_margin += 0.001f; });
    with([](Frame& g) { g.first_l += 0.25f; });
    with([](Frame& g) { g.cull = 0; });
    with([](Frame& g) { g.recs.pop_back(); });                       // n
    with([](Frame& g) { g.recs.push_back(g.recs[0]); });
    with([](Frame& g) { g.recs[3].cx += 0.5f; });
    with([](Frame& g) { g.recs[9].cy += 0.5f; });
    with([](Frame& g) { g.recs[0].cz += 0.5f; });
    with([](Frame& g) { g.recs[5].r += 0.5f; });
    with([](Frame& g) { g.recs[5].s_pass += 0.5f; });
    with([](Frame& g) { std::swap(g.recs[1], g.recs[2]); });         // reordered
    for (const Frame& g : changed) {
      EXPECT(!g.key().same(f.key()) && !f.key().same(g.key()));
      CullChain c;
      c.launch(f);
      c.launch(f);
      EXPECT(c.launch(f) == RayAction::kRead);
      EXPECT(c.launch(g) == RayAction::kTrace && c.last_ray == RayAction::kRead);
      EXPECT(c.caches.cull.valid && c.caches.cull.cached.same(f.key()));
      EXPECT(c.launch(f) == RayAction::kRead);   // back: the cache of f still serves
      EXPECT(c.launch(g) == RayAction::kTrace);
      EXPECT(c.launch(g) == RayAction::kFill && c.last_ray == RayAction::kRead);
      EXPECT(c.launch(g) == RayAction::kRead);
      EXPECT(c.launch(f) == RayAction::kTrace);  // f's bits are gone
      EXPECT(c.stats.cull_fills == 2 && c.dev.allocs == 4);
    }
    // one ulp of the camera position
    Frame u = f;
    uint32_t bits = sfrt::ray_key_bits(u.cam[1]) + 1u;
    std::memcpy(&u.cam[1], &bits, 4);
    EXPECT(!u.key().same(f.key()));
    // bit patterns: -0.0f is another key than 0.0f
    Frame z = f, nz = f;
    z.cam[0] = 0.0f;
    nz.cam[0] = -0.0f;
    EXPECT(!z.key().same(nz.key()) && z.key().same(z.key()));
  }
  {  // a field the cull does not read keeps the cache
    CullChain c;
    c.launch(f);
    c.launch(f);
    Frame g = f;
    g.recs[2].tex_off = 4096u;
    g.recs[2].tex_wh = 64u | (64u << 16);
    g.recs[7].atan_c += 1.0f;
    EXPECT(g.key().same(f.key()));
    EXPECT(c.launch(g) == RayAction::kRead);
    EXPECT(c.stats.cull_fills == 1 && c.stats.cull_hits == 1);
  }
  {  // a camera that walks every frame, or a sphere that moves every frame, never fills
    CullChain c;
    Frame g = f;
    for (int t = 0; t < 20; t++) {
      g.cam[2] += 0.01f;
      EXPECT(c.launch(g) == RayAction::kTrace);
    }
    for (int t = 0; t < 20; t++) {
      g.recs[4].cx += 0.01f;
      EXPECT(c.launch(g) == RayAction::kTrace);
    }
    EXPECT(c.last_ray == RayAction::kRead && c.stats.cull_fills == 0 && c.caches.cull_bytes() == 0 && c.dev.allocs == 2);
  }
  {  // a changed view: both caches miss, then both fill on the second launch
    CullChain c;
    c.launch(f);
    c.launch(f);
    c.launch(f);
    Frame g = f;
    g.ray.fwd[0] ^= 1u;
    EXPECT(c.launch(g) == RayAction::kTrace && c.last_ray == RayAction::kTrace);
    EXPECT(c.launch(g) == RayAction::kFill && c.last_ray == RayAction::kFill);
    EXPECT(c.launch(g) == RayAction::kRead);
    // the tile records were rewritten for g: f's cull cache cannot come back without a refill
    EXPECT(c.launch(f) == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill && c.last_ray == RayAction::kFill);
  }
  {  // a ray fill under a valid cull cache of another cull key drops that cache
    CullChain c;
    c.launch(f);
    c.launch(f);
    c.caches.invalidate();  // as SFRT_OPT_RAY_CACHE_MB = 0 does it
    EXPECT(c.launch(f) == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill);
    // and the policy on its own: the records refilled, the cull cache not -> not valid
    CullLayer p;
    p.commit(f.key(), RayAction::kFill, true);
    EXPECT(p.valid);
    Frame g = f;
    g.cam[0] += 1.0f;
    p.commit(g.key(), RayAction::kTrace, true);
    EXPECT(!p.valid);
    // a valid cull cache is not read by a launch that fills the ray cache
    CullLayer q;
    q.commit(f.key(), RayAction::kFill, true);
    EXPECT(q.decide(f.key(), RayAction::kRead, 100, 100, 0, kMiB) == RayAction::kRead);
    EXPECT(q.decide(f.key(), RayAction::kFill, 100, 100, 0, kMiB) == RayAction::kFill);
    EXPECT(q.decide(f.key(), RayAction::kTrace, 100, 100, 0, kMiB) == RayAction::kTrace);
  }
  {  // the budget: the cull cache's bytes count; a refused fill leaves the tile-record path
    const long long ray_bytes = sfrt::ray_cache_bytes(kTiles, 4);
    const long long cull_bytes = kTiles * 528;
    CullChain c;
    c.budget = ray_bytes + cull_bytes - 1;
    c.launch(f);
    EXPECT(c.launch(f) == RayAction::kTrace && c.last_ray == RayAction::kFill);
    EXPECT(c.launch(f) == RayAction::kTrace && c.last_ray == RayAction::kRead);
    EXPECT(c.caches.cull_bytes() == 0 && c.dev.allocs == 2);
    c.budget += 1;  // exactly fits
    EXPECT(c.launch(f) == RayAction::kFill && c.last_ray == RayAction::kRead);
    EXPECT(c.launch(f) == RayAction::kRead);
    EXPECT(c.caches.cull_bytes() == cull_bytes);
    CullChain d;  // other chains' bytes count
    d.budget = ray_bytes + cull_bytes + 1000;
    d.others = 1001;
    d.launch(f);
    EXPECT(d.launch(f) == RayAction::kTrace && d.last_ray == RayAction::kFill);
    d.others = 1000;
    EXPECT(d.launch(f) == RayAction::kFill);
    CullChain o;  // off
    o.budget = 0;
    for (int t = 0; t < 4; t++) EXPECT(o.launch(f) == RayAction::kTrace && o.last_ray == RayAction::kTrace);
    EXPECT(o.dev.allocs == 0);
    // a valid cache is not read once the option is 0
    EXPECT(c.caches.cull.decide(f.key(), RayAction::kRead, cull_bytes, cull_bytes, ray_bytes, 0) == RayAction::kTrace);
    // the list kernels' cache is larger and replaces the chain's buffers
    Frame big = f;
    big.recs = base_records(65);
    EXPECT(c.launch(big) == RayAction::kTrace);
    EXPECT(c.launch(big) == RayAction::kTrace);  // 12-byte lanes: past the budget
    c.budget += kTiles * 64 * 4;
    EXPECT(c.launch(big) == RayAction::kFill);
    EXPECT(c.caches.cull_wins.bytes == kTiles * 64 * 12 && c.dev.frees == 1);
  }
  {  // an allocation that fails: the launch culls for itself, the tile records stay readable
    CullChain c;
    c.launch(f);
    c.launch(f);
    Frame g = f;
    g.cam[0] += 1.0f;
    c.launch(g);
    Frame big = g;
    big.recs = base_records(100);
    c.launch(big);
    c.dev.fail_alloc = true;
    EXPECT(c.launch(big) == RayAction::kTrace && c.last_ray == RayAction::kRead);
    EXPECT(!c.caches.cull.valid && c.caches.ray.valid);
    c.dev.fail_alloc = false;
    EXPECT(c.launch(big) == RayAction::kFill);  // the next launch of the key tries again
    EXPECT(c.launch(big) == RayAction::kRead);
  }
  {  // a takeover by another stream: the chain's caches, buffers and layers, are kept
     // (TileSched::begin waits for the device; the caches never see the stream)
    CullChain c;
    c.launch(f);
    c.launch(f);
    const CullLayer before = c.caches.cull;
    EXPECT(c.launch(f) == RayAction::kRead);  // the launch of the other stream
    EXPECT(before.valid && c.caches.cull.valid && c.caches.cull.cached.same(before.cached));
  }
  {  // a failed launch invalidates both: first and second launch again
    CullChain c;
    c.launch(f);
    c.launch(f);
    EXPECT(c.launch(f, false) == RayAction::kRead);
    EXPECT(!c.caches.cull.valid && !c.caches.cull.have_prev && !c.caches.ray.valid);
    EXPECT(c.launch(f) == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill);
    CullChain d;  // a failed filling launch leaves no valid cache
    d.launch(f);
    EXPECT(d.launch(f, false) == RayAction::kFill);
    EXPECT(!d.caches.cull.valid);
    EXPECT(d.launch(f) == RayAction::kTrace);
    CullLayer p;
    p.commit(f.key(), RayAction::kFill, false);
    p.invalidate();
    EXPECT(!p.valid && !p.have_prev);
  }
  {  // the cull fill fails after the directions' fill of the same launch succeeded: the ray layer
     // commits as filled, the two above it are dropped, and the next launch refills them
    Chain c;  // (with a hit cache)
    const CullKey k = f.key();
    EXPECT(is(c.launch(k, kTiles, kRays), T, T, T));
    c.dev.fail_fill_cull = true;
    EXPECT(is(c.launch(k, kTiles, kRays), F, T, T));
    EXPECT(c.caches.ray.valid && c.caches.ray.cached.same(k.ray));
    EXPECT(!c.caches.cull.valid && !c.caches.hit.valid);
    EXPECT(c.stats.ray_fills == 1 && c.stats.ray_cached_frames == 1 && c.stats.cull_fills == 0 &&
           c.stats.hit_fills == 0);
    c.dev.fail_fill_cull = false;
    EXPECT(is(c.launch(k, kTiles, kRays), R, F, F));
    EXPECT(is(c.launch(k, kTiles, kRays), R, R, R));
    EXPECT(c.stats.ray_fills == 1 && c.stats.cull_fills == 1 && c.stats.hit_fills == 1 && c.stats.hit_hits == 1);
    // the directions' fill kernel failing: all three go, the launch traces
    Chain d;
    d.launch(k, kTiles, kRays);
    d.dev.fail_fill_rays = true;
    EXPECT(is(d.launch(k, kTiles, kRays), T, T, T));
    EXPECT(!d.caches.ray.valid && !d.caches.cull.valid && !d.caches.hit.valid);
    d.dev.fail_fill_rays = false;
    EXPECT(is(d.launch(k, kTiles, kRays), F, F, F));  // the launch was queued: its key is the previous one
  }
  {  // a refill of the directions frees the buffers that ride on the tile records before it
     // allocates, and the same launch fills them again
    Chain c;
    Frame g = f;
    for (int t = 0; t < 3; t++) c.launch(g.key(), kTiles, kRays);
    EXPECT(c.dev.allocs == 5 && c.dev.frees == 0);
    g.ray.fwd[0] ^= 1u;
    c.launch(g.key(), kTiles, kRays);
    EXPECT(c.caches.cull.valid && c.dev.frees == 0);  // a miss frees nothing: the old view may come back
    EXPECT(is(c.launch(g.key(), kTiles, kRays), F, F, F));
    EXPECT(c.dev.frees == 3 && c.dev.allocs == 8 && c.dev.live == 5);
  }
  if (failures) return 1;
  std::printf("cullcache_check ok\n");
  return 0;
}
