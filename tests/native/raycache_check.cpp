// raycache_check.cpp -- the policy of one cache layer (csrc/sfrt_raycache.h CacheLayer), as the
// directions' layer uses it, on the host: no HIP.
// Built and run by tests/test_ray_cache_policy.py (g++, with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sfrt_raycache.h"

using sfrt::RayAction;
using sfrt::RayKey;
using RayLayer = sfrt::CacheLayer<RayKey>;

static int failures = 0;
#define EXPECT(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

static RayKey base_key() {
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
  k.sub_w = 72; k.sub_row0 = 8; k.sub_rows = 12;
  k.tile_key = (1ll << 62) | (2ll << 56) | (5ll << 28) | 2;
  return k;
}

constexpr long long kMiB = 1ll << 20;

// One launch as ChainCaches makes it for the layer with none below: decide, then commit the
// decision -- or, the launch having failed, invalidate.
static RayAction launch(RayLayer& p, const RayKey& k, long long bytes = 1000,
                        long long held = 0, long long others = 0, long long budget = 512 * kMiB,
                        bool queued = true) {
  const RayAction a = p.decide(k, RayAction::kRead, bytes, held, others, budget);
  if (queued) p.commit(k, a, false);
  else p.invalidate();
  return a;
}

// Every single-field change of the key, one at a time.
static std::vector<RayKey> single_field_changes(const RayKey& k) {
  std::vector<RayKey> out;
  auto with = [&](auto&& change) {
    RayKey c = k;
    change(c);
    out.push_back(c);
  };
  for (int q = 0; q < 3; q++) {
    with([&](RayKey& c) { c.fwd[q] ^= 1u; });
    with([&](RayKey& c) { c.right[q] ^= 1u; });
    with([&](RayKey& c) { c.up[q] ^= 0x80000000u; });  // -0.0f is another key than 0.0f
  }
  with([](RayKey& c) { c.h_start ^= 1u; });
  with([](RayKey& c) { c.h_inc ^= 1u; });
  with([](RayKey& c) { c.v_start ^= 1u; });
  with([](RayKey& c) { c.v_inc ^= 1u; });
  with([](RayKey& c) { c.xstart += 1; });
  with([](RayKey& c) { c.xadd += 1; });
  with([](RayKey& c) { c.ystart += 1; });
  with([](RayKey& c) { c.yadd += 1; });
  with([](RayKey& c) { c.sub_w += 1; });
  with([](RayKey& c) { c.sub_row0 += 8; });
  with([](RayKey& c) { c.sub_rows += 1; });
  with([](RayKey& c) { c.tile_key ^= 1ll << 59; });  // the supersampling factor
  with([](RayKey& c) { c.tile_key ^= 1ll << 56; });  // pixels per lane
  with([](RayKey& c) { c.tile_key += 1; });          // the grid
  return out;
}

int main() {
  const RayKey k = base_key();
  {  // fill only on the second consecutive equal key, read from then on
    RayLayer p;
    EXPECT(launch(p, k) == RayAction::kTrace);
    EXPECT(!p.valid);
    EXPECT(launch(p, k) == RayAction::kFill);
    EXPECT(p.valid);
    EXPECT(launch(p, k) == RayAction::kRead);
    EXPECT(launch(p, k) == RayAction::kRead);
  }
  {  // a miss on each single key field; the cache survives it and serves the old key again
    const std::vector<RayKey> changed = single_field_changes(k);
    EXPECT(changed.size() == 23);
    for (const RayKey& c : changed) {
      EXPECT(!c.same(k) && !k.same(c));
      RayLayer p;
      launch(p, k);
      launch(p, k);
      EXPECT(launch(p, c) == RayAction::kTrace);  // no read of another key's directions
      EXPECT(p.valid && p.cached.same(k));
      EXPECT(launch(p, k) == RayAction::kRead);   // turning back
      EXPECT(launch(p, c) == RayAction::kTrace);
      EXPECT(launch(p, c) == RayAction::kFill);   // the second consecutive one rebuilds
      EXPECT(p.cached.same(c));
      EXPECT(launch(p, k) == RayAction::kTrace);  // the old key's directions are gone
    }
  }
  {  // a camera that turns every frame never fills
    RayLayer p;
    for (uint32_t t = 0; t < 100; t++) {
      RayKey c = k;
      c.fwd[0] = t;
      c.right[2] = t * 7u;
      EXPECT(launch(p, c) == RayAction::kTrace);
      EXPECT(!p.valid);
    }
    // nor do two keys taking turns (two bands through one chain)
    RayKey c = k;
    c.sub_row0 += 16;
    for (int t = 0; t < 10; t++) EXPECT(launch(p, t % 2 ? c : k) == RayAction::kTrace);
  }
  {  // the budget: a fill past it is refused, and the frame renders as without the cache
    RayLayer p;
    launch(p, k);
    EXPECT(launch(p, k, 2 * kMiB, 0, 0, 1 * kMiB) == RayAction::kTrace);
    EXPECT(!p.valid);
    EXPECT(launch(p, k, 2 * kMiB, 0, 0, 2 * kMiB) == RayAction::kFill);  // exactly the budget fits
    RayLayer q;
    launch(q, k);
    EXPECT(launch(q, k, 2 * kMiB, 0, 3 * kMiB, 4 * kMiB) == RayAction::kTrace);  // other chains count
    EXPECT(launch(q, k, 2 * kMiB, 0, 2 * kMiB, 4 * kMiB) == RayAction::kFill);
    // a smaller cache into the chain's larger buffer keeps that buffer: its size counts
    RayLayer r;
    launch(r, k);
    EXPECT(launch(r, k, 1 * kMiB, 3 * kMiB, 2 * kMiB, 4 * kMiB) == RayAction::kTrace);
    EXPECT(launch(r, k, 1 * kMiB, 3 * kMiB, 1 * kMiB, 4 * kMiB) == RayAction::kFill);
    // off
    RayLayer o;
    for (int t = 0; t < 4; t++) EXPECT(launch(o, k, 1000, 0, 0, 0) == RayAction::kTrace);
    // a valid cache is not read once the option is 0
    EXPECT(p.valid && p.decide(k, RayAction::kRead, 2 * kMiB, 2 * kMiB, 0, 0) == RayAction::kTrace);
  }
  {  // a failed launch invalidates: the next two launches are a first and a second one again
    RayLayer p;
    launch(p, k);
    launch(p, k);
    EXPECT(launch(p, k, 1000, 1000, 0, 512 * kMiB, false) == RayAction::kRead);
    EXPECT(!p.valid && !p.have_prev);
    EXPECT(launch(p, k) == RayAction::kTrace);
    EXPECT(launch(p, k) == RayAction::kFill);
    // a failed filling launch leaves no valid cache either
    RayLayer q;
    launch(q, k);
    EXPECT(launch(q, k, 1000, 0, 0, 512 * kMiB, false) == RayAction::kFill);
    EXPECT(!q.valid);
    EXPECT(launch(q, k) == RayAction::kTrace);
  }
  EXPECT(sfrt::ray_cache_bytes(32400, 4) == 32400ll * 4 * 64 * 12);
  if (failures) return 1;
  std::printf("raycache_check ok\n");
  return 0;
}
