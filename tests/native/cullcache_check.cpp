// cullcache_check.cpp -- the cull cache's policy (csrc/sfrt_raycache.h CullKey, CullCachePolicy)
// on the host: no HIP.  A chain is modelled as the world drives it (sfrt_world.cpp sched_begin /
// sched_end): the ray cache decides first, then the cull cache; a fill reserves the chain's
// CacheBufs through counting allocators.  Built and run by tests/test_cull_cache_policy.py (g++,
// with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "sfrt_raycache.h"

using sfrt::CacheBuf;
using sfrt::CullCachePolicy;
using sfrt::CullKey;
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

// sfrt_trace.h SphereRec's members, so that the key's field list is checked against the record
// the kernels read (the header itself needs no HIP, but this test needs only the names).
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

// A launch's frame as far as the cull reads it.
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

// One chain and the world's budget around it, with counting allocators.
struct Chain {
  RayCachePolicy ray;
  CullCachePolicy cull;
  CacheBuf ray_dirs, cull_recs, cull_wins;
  long long budget = 512 * kMiB, others = 0;
  int allocs = 0, frees = 0, live = 0;
  bool alloc_fails = false;
  int cull_fills = 0, cull_hits = 0;
  RayAction last_ray = RayAction::kTrace;

  ~Chain() {
    for (CacheBuf* b : {&ray_dirs, &cull_recs, &cull_wins}) b->release([this](void* p) { return free_fn(p); });
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
  void* alloc_fn(long long n) {
    if (alloc_fails) return nullptr;
    allocs++;
    live++;
    return std::malloc((size_t)n);
  }
  bool reserve(CacheBuf& b, long long n) {
    return b.reserve(n, [this](void* p) { return free_fn(p); }, [this](long long m) { return alloc_fn(m); });
  }
  long long cull_bytes() const { return cull_recs.bytes + cull_wins.bytes; }

  // sched_begin and sched_end of one launch; returns the cull cache's action.
  RayAction launch(const Frame& f, bool queued = true) {
    const RayKey rk = f.ray;
    const long long ray_bytes = sfrt::ray_cache_bytes(kTiles, 4);
    RayAction ra = ray.decide(rk, ray_bytes, ray_dirs.bytes, others, budget);
    if (ra == RayAction::kFill) {  // the tile records are rewritten: the cull cache under them goes first
      for (CacheBuf* b : {&cull_recs, &cull_wins}) b->release([this](void* p) { return free_fn(p); });
      cull.valid = false;
    }
    if (ra == RayAction::kFill && !reserve(ray_dirs, ray_bytes)) {
      ray.invalidate();
      cull.invalidate();
      ra = RayAction::kTrace;
    }
    const CullKey ck = f.key();
    const bool list = ck.n > 64;
    const long long rb = sfrt::cull_rec_bytes(kTiles), wb = sfrt::cull_win_bytes(kTiles, list);
    RayAction ca = cull.decide(ck, ra, rb + wb, cull_bytes(), others + ray_dirs.bytes, budget);
    if (ca == RayAction::kFill && !(reserve(cull_recs, rb) && reserve(cull_wins, wb))) {
      cull.invalidate();
      ca = RayAction::kTrace;
    }
    if (!queued) {  // TileSched::end: both go
      ray.invalidate();
      cull.invalidate();
    } else {
      ray.commit(rk, ra, true);
      cull.commit(ck, ra, ca, true);
      if (ca == RayAction::kFill) cull_fills++;
      if (ca == RayAction::kRead) cull_hits++;
    }
    // the cull cache is never valid without valid tile records
    EXPECT(!cull.valid || ray.valid);
    EXPECT(ca == RayAction::kTrace || ra != RayAction::kTrace);
    last_ray = ra;
    return ca;
  }
};

int main() {
  const Frame f;
  EXPECT(sizeof(sfrt::CullRec) + 64 * sizeof(sfrt::CullWin) == 528);
  EXPECT(sfrt::cull_rec_bytes(32400) + sfrt::cull_win_bytes(32400, false) == 32400ll * 528);
  EXPECT(sfrt::cull_win_bytes(3, true) == 3 * 64 * 12);
  {  // fill on the second identical key (with the ray cache's fill), read on the third
    Chain c;
    EXPECT(c.launch(f) == RayAction::kTrace && c.last_ray == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill && c.last_ray == RayAction::kFill);
    EXPECT(c.cull_fills == 1 && c.cull_hits == 0 && c.allocs == 3);
    EXPECT(c.launch(f) == RayAction::kRead && c.last_ray == RayAction::kRead);
    EXPECT(c.launch(f) == RayAction::kRead);
    EXPECT(c.cull_fills == 1 && c.cull_hits == 2 && c.allocs == 3 && c.frees == 0);
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
      Chain c;
      c.launch(f);
      c.launch(f);
      EXPECT(c.launch(f) == RayAction::kRead);
      EXPECT(c.launch(g) == RayAction::kTrace && c.last_ray == RayAction::kRead);
      EXPECT(c.cull.valid && c.cull.cached.same(f.key()));
      EXPECT(c.launch(f) == RayAction::kRead);   // back: the cache of f still serves
      EXPECT(c.launch(g) == RayAction::kTrace);
      EXPECT(c.launch(g) == RayAction::kFill && c.last_ray == RayAction::kRead);
      EXPECT(c.launch(g) == RayAction::kRead);
      EXPECT(c.launch(f) == RayAction::kTrace);  // f's bits are gone
      EXPECT(c.cull_fills == 2 && c.allocs == 3);
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
    Chain c;
    c.launch(f);
    c.launch(f);
    Frame g = f;
    g.recs[2].tex_off = 4096u;
    g.recs[2].tex_wh = 64u | (64u << 16);
    g.recs[7].atan_c += 1.0f;
    EXPECT(g.key().same(f.key()));
    EXPECT(c.launch(g) == RayAction::kRead);
    EXPECT(c.cull_fills == 1 && c.cull_hits == 1);
  }
  {  // a camera that walks every frame, or a sphere that moves every frame, never fills
    Chain c;
    Frame g = f;
    for (int t = 0; t < 20; t++) {
      g.cam[2] += 0.01f;
      EXPECT(c.launch(g) == RayAction::kTrace);
    }
    for (int t = 0; t < 20; t++) {
      g.recs[4].cx += 0.01f;
      EXPECT(c.launch(g) == RayAction::kTrace);
    }
    EXPECT(c.last_ray == RayAction::kRead && c.cull_fills == 0 && c.cull_bytes() == 0 && c.allocs == 1);
  }
  {  // a changed view: both caches miss, then both fill on the second launch
    Chain c;
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
    Chain c;
    c.launch(f);
    c.launch(f);
    c.ray.invalidate();  // as sfrt_world.cpp does it: both
    c.cull.invalidate();
    EXPECT(c.launch(f) == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill);
    // and the policy on its own: the records refilled, the cull cache not -> not valid
    CullCachePolicy p;
    p.commit(f.key(), RayAction::kFill, RayAction::kFill, true);
    EXPECT(p.valid);
    Frame g = f;
    g.cam[0] += 1.0f;
    p.commit(g.key(), RayAction::kFill, RayAction::kTrace, true);
    EXPECT(!p.valid);
    // a valid cull cache is not read by a launch that fills the ray cache
    CullCachePolicy q;
    q.commit(f.key(), RayAction::kFill, RayAction::kFill, true);
    EXPECT(q.decide(f.key(), RayAction::kRead, 100, 100, 0, kMiB) == RayAction::kRead);
    EXPECT(q.decide(f.key(), RayAction::kFill, 100, 100, 0, kMiB) == RayAction::kFill);
    EXPECT(q.decide(f.key(), RayAction::kTrace, 100, 100, 0, kMiB) == RayAction::kTrace);
  }
  {  // the budget: the cull cache's bytes count; a refused fill leaves the tile-record path
    const long long ray_bytes = sfrt::ray_cache_bytes(kTiles, 4);
    const long long cull_bytes = kTiles * 528;
    Chain c;
    c.budget = ray_bytes + cull_bytes - 1;
    c.launch(f);
    EXPECT(c.launch(f) == RayAction::kTrace && c.last_ray == RayAction::kFill);
    EXPECT(c.launch(f) == RayAction::kTrace && c.last_ray == RayAction::kRead);
    EXPECT(c.cull_bytes() == 0 && c.allocs == 1);
    c.budget += 1;  // exactly fits
    EXPECT(c.launch(f) == RayAction::kFill && c.last_ray == RayAction::kRead);
    EXPECT(c.launch(f) == RayAction::kRead);
    EXPECT(c.cull_bytes() == cull_bytes);
    Chain d;  // other chains' bytes count
    d.budget = ray_bytes + cull_bytes + 1000;
    d.others = 1001;
    d.launch(f);
    EXPECT(d.launch(f) == RayAction::kTrace && d.last_ray == RayAction::kFill);
    d.others = 1000;
    EXPECT(d.launch(f) == RayAction::kFill);
    Chain o;  // off
    o.budget = 0;
    for (int t = 0; t < 4; t++) EXPECT(o.launch(f) == RayAction::kTrace && o.last_ray == RayAction::kTrace);
    EXPECT(o.allocs == 0);
    // a valid cache is not read once the option is 0
    EXPECT(c.cull.decide(f.key(), RayAction::kRead, cull_bytes, cull_bytes, ray_bytes, 0) == RayAction::kTrace);
    // the list kernels' cache is larger and replaces the chain's buffers
    Frame big = f;
    big.recs = base_records(65);
    EXPECT(c.launch(big) == RayAction::kTrace);
    EXPECT(c.launch(big) == RayAction::kTrace);  // 12-byte lanes: past the budget
    c.budget += kTiles * 64 * 4;
    EXPECT(c.launch(big) == RayAction::kFill);
    EXPECT(c.cull_wins.bytes == kTiles * 64 * 12 && c.frees == 1);
  }
  {  // an allocation that fails: the launch culls for itself, the tile records stay readable
    Chain c;
    c.launch(f);
    c.launch(f);
    Frame g = f;
    g.cam[0] += 1.0f;
    c.launch(g);
    Frame big = g;
    big.recs = base_records(100);
    c.launch(big);
    c.alloc_fails = true;
    EXPECT(c.launch(big) == RayAction::kTrace && c.last_ray == RayAction::kRead);
    EXPECT(!c.cull.valid && c.ray.valid);
    c.alloc_fails = false;
    EXPECT(c.launch(big) == RayAction::kFill);  // the next launch of the key tries again
    EXPECT(c.launch(big) == RayAction::kRead);
  }
  {  // a takeover by another stream: the chain object, its buffers and both policies are kept
     // (TileSched::begin waits for the device and changes neither policy)
    Chain c;
    c.launch(f);
    c.launch(f);
    const CullCachePolicy before = c.cull;
    EXPECT(c.launch(f) == RayAction::kRead);  // the launch of the other stream
    EXPECT(before.valid && c.cull.valid && c.cull.cached.same(before.cached));
  }
  {  // a failed launch invalidates both: first and second launch again
    Chain c;
    c.launch(f);
    c.launch(f);
    EXPECT(c.launch(f, false) == RayAction::kRead);
    EXPECT(!c.cull.valid && !c.cull.have_prev && !c.ray.valid);
    EXPECT(c.launch(f) == RayAction::kTrace);
    EXPECT(c.launch(f) == RayAction::kFill);
    Chain d;  // a failed filling launch leaves no valid cache
    d.launch(f);
    EXPECT(d.launch(f, false) == RayAction::kFill);
    EXPECT(!d.cull.valid);
    EXPECT(d.launch(f) == RayAction::kTrace);
    CullCachePolicy p;
    p.commit(f.key(), RayAction::kRead, RayAction::kFill, false);
    EXPECT(!p.valid && !p.have_prev);
  }
  if (failures) return 1;
  std::printf("cullcache_check ok\n");
  return 0;
}
