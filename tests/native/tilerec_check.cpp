// tilerec_check.cpp -- the tile records of the ray cache (csrc/sfrt_raycache.h) on the host: the
// record's layout as the fill kernel and the trace kernels both see it through that one header,
// and a chain's allocate / keep / invalidate bookkeeping of the directions' and the records'
// buffers, through ChainCaches::begin / end (chain_harness.h) under a walking camera -- the cull
// key changes with every launch, so only the ray layer ever acts.  No HIP.
// Built and run by tests/test_tile_record_layout.py (g++, with -fsanitize=address,undefined).
#include <cstddef>
#include <type_traits>

#include "chain_harness.h"

using sfrt::TileRec;

// The layout the kernels rely on: eight dwords in this order, one aligned 32-byte load.
static_assert(std::is_standard_layout<TileRec>::value && std::is_trivially_copyable<TileRec>::value,
              "a plain record");
static_assert(sizeof(TileRec) == 32 && alignof(TileRec) == 32, "size and alignment");
static_assert(offsetof(TileRec, ax) == 0 && offsetof(TileRec, ay) == 4 && offsetof(TileRec, az) == 8,
              "the axis");
static_assert(offsetof(TileRec, sin_t) == 12 && offsetof(TileRec, cos_t) == 16, "the half-angle");
static_assert(offsetof(TileRec, wide) == 20, "the wide flag");
static_assert(offsetof(TileRec, tile_x) == 24 && offsetof(TileRec, tile_y) == 28, "the grid position");
static_assert(sizeof(((TileRec*)nullptr)->wide) == 4 && sizeof(((TileRec*)nullptr)->tile_x) == 4 &&
                  sizeof(((TileRec*)nullptr)->sin_t) == 4,
              "binary32 and u32 fields");

using Heap = Device;

// One chain whose camera walks: every launch's cull key is another one.
struct WalkingChain : Chain {
  uint32_t step = 0;
  explicit WalkingChain(Heap* h) : Chain(*h) {}

  // what the launch reads: both buffers, or neither
  struct Launch {
    RayAction action;
    const void* dirs;
    const void* recs;
  };
  Launch launch(const RayKey& k, long long tiles, int rays, long long ray_budget = 512 * kMiB,
                bool queued = true) {
    budget = ray_budget;
    CullKey ck;
    ck.ray = k;
    ck.cam[0] = step++;
    const TraceCaches d = Chain::launch(ck, tiles, rays, queued);
    EXPECT(d.cull == T && d.hit == T && caches.cull_bytes() == 0 && caches.hit_bytes() == 0);
    return Launch{d.ray, d.dirs, d.tile_recs};
  }
};

static RayKey key_of(long long tiles_x, long long tiles_y, int rays, uint32_t fwd0 = 0) {
  RayKey k{};
  k.fwd[0] = fwd0;
  k.fwd[2] = sfrt::ray_key_bits(1.0f);
  k.right[0] = sfrt::ray_key_bits(1.0f);
  k.up[1] = sfrt::ray_key_bits(-1.0f);
  k.h_inc = sfrt::ray_key_bits(0.01f);
  k.v_inc = sfrt::ray_key_bits(0.02f);
  k.xadd = 1; k.yadd = 1;
  k.sub_w = (int32_t)(tiles_x * rays * 8); k.sub_rows = (int32_t)(tiles_y * 8);
  k.tile_key = (1ll << 62) | ((long long)rays << 56) | (tiles_x << 28) | tiles_y;
  return k;
}

int main() {
  EXPECT(sfrt::tile_rec_bytes(0) == 0);
  EXPECT(sfrt::tile_rec_bytes(28) == 28 * 32);
  EXPECT(sfrt::tile_rec_bytes(32400) == 32400ll * 32);  // 4K at four pixels per lane: 1.04 MB
  EXPECT(sfrt::tile_rec_bytes(1ll << 28) == 1ll << 33);  // the largest ordered grid: no 32-bit wrap
  // the directions' figure is unchanged: the records are counted apart
  EXPECT(sfrt::ray_cache_bytes(32400, 4) == 32400ll * 4 * 64 * 12);
  {  // an array of records keeps every element aligned and contiguous
    TileRec* a = new TileRec[3]();
    EXPECT(((uintptr_t)&a[0] & 31u) == 0 && (char*)&a[2] - (char*)&a[0] == 64);
    a[1].wide = 1u;
    a[1].tile_x = 5u;
    const uint32_t* w = (const uint32_t*)&a[1];
    EXPECT(w[5] == 1u && w[6] == 5u && w[7] == 0u);
    delete[] a;
  }
  Heap heap;
  {  // allocate with the fill, keep while the key is read, keep on a position change
    WalkingChain c(&heap);
    const RayKey k = key_of(4, 7, 4);
    WalkingChain::Launch l = c.launch(k, 28, 4);
    EXPECT(l.action == RayAction::kTrace && !l.dirs && !l.recs);
    EXPECT(c.caches.dirs.bytes == 0 && c.caches.tile_recs.bytes == 0 && heap.allocs == 0);
    l = c.launch(k, 28, 4);
    EXPECT(l.action == RayAction::kFill && l.dirs && l.recs);
    EXPECT(c.caches.dirs.bytes == sfrt::ray_cache_bytes(28, 4) && c.caches.tile_recs.bytes == 28 * 32);
    EXPECT(heap.allocs == 2 && heap.frees == 0);
    const void* d0 = c.caches.dirs.ptr;
    const void* r0 = c.caches.tile_recs.ptr;
    for (int t = 0; t < 3; t++) {  // the key holds no camera position: walking reads
      l = c.launch(k, 28, 4);
      EXPECT(l.action == RayAction::kRead && l.dirs == d0 && l.recs == r0);
    }
    EXPECT(heap.allocs == 2 && heap.frees == 0);
    // a basis change: the records are dropped with the directions (no read), the buffers stay
    const RayKey turned = key_of(4, 7, 4, 7u);
    l = c.launch(turned, 28, 4);
    EXPECT(l.action == RayAction::kTrace && !l.dirs && !l.recs);
    l = c.launch(turned, 28, 4);  // refilled into the same buffers
    EXPECT(l.action == RayAction::kFill && l.dirs == d0 && l.recs == r0);
    EXPECT(heap.allocs == 2 && heap.frees == 0);
    EXPECT(c.launch(k, 28, 4).action == RayAction::kTrace);  // the old key's records are gone
    // a smaller grid fits both buffers as they are
    const RayKey small = key_of(2, 3, 4);
    c.launch(small, 6, 4);
    l = c.launch(small, 6, 4);
    EXPECT(l.action == RayAction::kFill && l.recs == r0 && c.caches.tile_recs.bytes == 28 * 32);
    EXPECT(heap.allocs == 2 && heap.frees == 0);
    // a larger grid: both are replaced, old ones freed first
    const RayKey large = key_of(13, 30, 4);
    c.launch(large, 390, 4);
    l = c.launch(large, 390, 4);
    EXPECT(l.action == RayAction::kFill && l.dirs && l.recs);
    EXPECT(c.caches.dirs.bytes == sfrt::ray_cache_bytes(390, 4) && c.caches.tile_recs.bytes == 390 * 32);
    EXPECT(heap.allocs == 4 && heap.frees == 2);
    // more tiles at fewer pixels per lane: fewer direction bytes, more record bytes -- only the
    // records grow
    const RayKey narrow = key_of(50, 30, 1);
    EXPECT(sfrt::ray_cache_bytes(1500, 1) < c.caches.dirs.bytes && sfrt::tile_rec_bytes(1500) > c.caches.tile_recs.bytes);
    const void* d1 = c.caches.dirs.ptr;
    c.launch(narrow, 1500, 1);
    l = c.launch(narrow, 1500, 1);
    EXPECT(l.action == RayAction::kFill && l.dirs == d1 && c.caches.tile_recs.bytes == 1500 * 32);
    EXPECT(heap.allocs == 5 && heap.frees == 3);
    // a failed launch invalidates both: nothing is read until the second equal launch refills
    l = c.launch(narrow, 1500, 1, 512 * kMiB, false);
    EXPECT(l.action == RayAction::kRead);
    EXPECT(!c.caches.ray.valid);
    l = c.launch(narrow, 1500, 1);
    EXPECT(l.action == RayAction::kTrace && !l.recs);
    l = c.launch(narrow, 1500, 1);
    EXPECT(l.action == RayAction::kFill && l.recs == c.caches.tile_recs.ptr);
    EXPECT(heap.allocs == 5 && heap.frees == 3);  // into the buffers it still holds
    // the option at 0: no read, no fill; the records do not count against a budget that the
    // directions exactly fill
    EXPECT(c.launch(narrow, 1500, 1, 0).action == RayAction::kTrace);
    c.release();
    EXPECT(c.caches.dirs.bytes == 0 && c.caches.tile_recs.bytes == 0 && !c.caches.dirs.ptr && !c.caches.tile_recs.ptr);
    EXPECT(heap.allocs == 5 && heap.frees == 5);
    c.launch(k, 28, 4, sfrt::ray_cache_bytes(28, 4));
    EXPECT(c.launch(k, 28, 4, sfrt::ray_cache_bytes(28, 4)).action == RayAction::kFill);
    EXPECT(c.launch(k, 28, 4, sfrt::ray_cache_bytes(28, 4) - 1).action == RayAction::kRead);
  }
  EXPECT(heap.allocs == 7 && heap.frees == 7);
  {  // no memory for the records: the launch renders uncached and reads neither buffer
    Heap h;
    WalkingChain c(&h);
    const RayKey k = key_of(4, 7, 4);
    c.launch(k, 28, 4);
    h.fail_alloc = true;
    WalkingChain::Launch l = c.launch(k, 28, 4);
    EXPECT(l.action == RayAction::kTrace && !l.dirs && !l.recs && !c.caches.ray.valid);
    EXPECT(c.caches.dirs.bytes == 0 && c.caches.tile_recs.bytes == 0);
    h.fail_alloc = false;
    // the launch itself was queued and committed its key: the next equal one tries again
    l = c.launch(k, 28, 4);
    EXPECT(l.action == RayAction::kFill && l.dirs && l.recs && c.caches.tile_recs.bytes == 28 * 32);
    // a free that fails keeps the old buffer and its size, and fills nothing
    const RayKey large = key_of(13, 30, 4);
    c.launch(large, 390, 4);
    h.fail_free = true;
    l = c.launch(large, 390, 4);
    EXPECT(l.action == RayAction::kTrace && c.caches.dirs.bytes == sfrt::ray_cache_bytes(28, 4) && c.caches.dirs.ptr);
    h.fail_free = false;
  }
  {  // two chains: each its own records
    Heap h;
    WalkingChain a(&h), b(&h);
    const RayKey k = key_of(4, 7, 4);
    for (int t = 0; t < 3; t++) {
      a.launch(k, 28, 4);
      b.launch(k, 28, 4);
    }
    EXPECT(a.caches.tile_recs.ptr && b.caches.tile_recs.ptr && a.caches.tile_recs.ptr != b.caches.tile_recs.ptr && a.caches.dirs.ptr != b.caches.dirs.ptr);
    EXPECT(a.caches.tile_recs.bytes + b.caches.tile_recs.bytes == 2 * 28 * 32);
  }
  if (failures) return 1;
  std::printf("tilerec_check ok\n");
  return 0;
}
