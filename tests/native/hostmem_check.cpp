// hostmem_check.cpp -- the host layer's HIP-free helpers (csrc/sfrt_hostmem.h) on the host: the
// ray batches' staging layout against the offsets each host call used to compute by hand, the
// subset scatter against a per-pixel loop, grown_capacity, and CacheBuf's state after a failed
// free and a failed allocation.  No HIP.
// Built and run by tests/test_hostmem.py (g++, with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sfrt_hostmem.h"

using sfrt::BatchLayout;
using sfrt::BatchPart;
using sfrt::CacheBuf;

static int failures = 0;
#define EXPECT(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

// The outputs' offsets as every host call computed them: back to back from in_bytes, an absent
// output taking no room.  Returns the total.
static size_t outputs_by_hand(size_t n, size_t in_bytes, const bool* want, const size_t* elem, int count,
                              size_t* off) {
  size_t bytes = in_bytes;
  for (int q = 0; q < count; q++) {
    off[q] = bytes;
    if (want[q]) bytes += n * elem[q];
  }
  return bytes;
}

// One layout against the by-hand figures: in_off / in_want for the inputs, the outputs from
// outputs_by_hand.  Then a round trip through a staging buffer of exactly `bytes` bytes (the
// address sanitizer sees a byte too many): inputs in, outputs out, but for the skipped one.
static void check_layout(size_t n, const std::vector<BatchPart>& in, const std::vector<size_t>& in_off,
                         size_t in_bytes, const std::vector<size_t>& elem, unsigned mask) {
  const int no = (int)elem.size();
  std::vector<std::vector<uint8_t>> host(no);
  bool want[BatchLayout::kMaxParts] = {};
  BatchPart out[BatchLayout::kMaxParts] = {};
  for (int q = 0; q < no; q++) {
    want[q] = (mask >> q) & 1u;
    host[q].assign(n * elem[q], 0);
    out[q] = {want[q] ? host[q].data() : nullptr, elem[q]};
  }
  size_t off[BatchLayout::kMaxParts];
  const size_t bytes = outputs_by_hand(n, in_bytes, want, elem.data(), no, off);
  // (initializer lists have a static length: one spelling per count of parts)
  const auto lay = [&]() {
    const BatchPart* i = in.data();
    const BatchPart* o = out;
    if (in.size() == 1) return BatchLayout(n, {i[0]}, {o[0], o[1], o[2], o[3], o[4]});
    if (in.size() == 2) return BatchLayout(n, {i[0], i[1]}, {o[0], o[1], o[2], o[3], o[4]});
    if (no == 2) return BatchLayout(n, {i[0], i[1], i[2]}, {o[0], o[1]});
    return BatchLayout(n, {i[0], i[1], i[2]}, {o[0], o[1], o[2], o[3], o[4], o[5]});
  };
  const BatchLayout l = lay();
  EXPECT(l.n == n && l.n_in == (int)in.size() && l.n_out == no);
  EXPECT(l.in_bytes == in_bytes && l.bytes == bytes);
  std::vector<uint8_t> stage(bytes, 0xee);
  for (size_t q = 0; q < in.size(); q++) {
    if (in[q].host) EXPECT(l.in_off[q] == in_off[q]);
    EXPECT(l.in_at<uint8_t>(stage.data(), (int)q) == (in[q].host ? stage.data() + in_off[q] : nullptr));
  }
  for (int q = 0; q < no; q++) {
    if (want[q]) EXPECT(l.out_off[q] == off[q]);
    EXPECT(l.out_at<uint8_t>(stage.data(), q) == (want[q] ? stage.data() + off[q] : nullptr));
  }
  l.stage_inputs(stage.data());
  for (size_t q = 0; q < in.size(); q++)
    if (in[q].host) EXPECT(std::memcmp(stage.data() + in_off[q], in[q].host, n * in[q].elem) == 0);
  for (size_t b = in_bytes; b < bytes; b++) stage[b] = (uint8_t)(b * 7 + 1);
  const int skipped = no - 1;  // the sphere world's rule under SFRT_E_TEXEL: all but rgba
  l.copy_outputs(stage.data(), 1u << skipped);
  for (int q = 0; q < no; q++) {
    bool copied = true, untouched = true;
    for (size_t b = 0; b < n * elem[q]; b++) {
      copied = copied && want[q] && host[q][b] == (uint8_t)((off[q] + b) * 7 + 1);
      untouched = untouched && host[q][b] == 0;
    }
    EXPECT((want[q] && q != skipped) ? copied : untouched);
  }
  l.copy_outputs(stage.data());
  if (want[skipped]) EXPECT(host[skipped][0] == (uint8_t)(off[skipped] * 7 + 1));
}

static void check_layouts() {
  const size_t sizes[3] = {1, 63, 65};
  for (size_t n : sizes) {
    std::vector<float> a(n * 3, 1.5f), b(n * 3, 2.5f), c(n * 3, 3.5f);
    const std::vector<size_t> hits5 = {12, 4, 4, 4, 4}, hits6 = {12, 4, 4, 4, 4, 4}, shadow = {4, 4};
    for (unsigned mask = 0; mask < 64; mask++) {
      if (mask < 32) {
        // the sphere world: dirs, then origins when given (in_bytes = n * 12 * (origins ? 2 : 1))
        check_layout(n, {{a.data(), 12}, {b.data(), 12}}, {0, n * 12}, n * 24, hits5, mask);
        check_layout(n, {{a.data(), 12}, {nullptr, 12}}, {0, 0}, n * 12, hits5, mask);
        // GLSL: dirs alone
        check_layout(n, {{a.data(), 12}}, {0}, n * 12, hits5, mask);
      }
      // voxel: dirs, yscales, origins (off_ys = n * 12, off_org = off_ys + (yscales ? n * 4 : 0))
      for (int ys = 0; ys < 2; ys++)
        for (int org = 0; org < 2; org++) {
          const size_t off_org = n * 12 + (ys ? n * 4 : 0);
          check_layout(n, {{a.data(), 12}, {ys ? b.data() : nullptr, 4}, {org ? c.data() : nullptr, 12}},
                       {0, n * 12, off_org}, off_org + (org ? n * 12 : 0), hits6, mask);
        }
      // shadow: origins, dirs, max_dists (in_bytes = n * 28), then free and steps
      if (mask < 4)
        check_layout(n, {{a.data(), 12}, {b.data(), 12}, {c.data(), 4}}, {0, n * 12, n * 24}, n * 28,
                     shadow, mask);
    }
  }
}

// The scatter against the per-pixel loop, on a 7x5 frame with 64 guard bytes on either side.
static void check_scatter() {
  const int W = 7, H = 5, guard = 64;
  const size_t frame = (size_t)W * H * 4;
  struct Case { int xstart, xadd, ystart, yadd; };
  std::vector<Case> cases;
  for (int xadd : {1, 3})
    for (int yadd : {1, 2})
      for (int xs : {0, 1})
        for (int ys : {0, 1}) cases.push_back({xs, xadd, ys, yadd});
  cases.push_back({3, W, 0, 1});  // one column (a stride that addresses one pixel per row)
  cases.push_back({0, 1, 2, H});  // one row
  cases.push_back({6, 1, 4, 1});  // the last pixel
  for (const Case& c : cases) {
    const int sub_w = (W - c.xstart + c.xadd - 1) / c.xadd, sub_h = (H - c.ystart + c.yadd - 1) / c.yadd;
    std::vector<uint32_t> src((size_t)sub_w * sub_h);
    for (size_t k = 0; k < src.size(); k++) src[k] = 0x01020304u * (uint32_t)(k + 1);
    std::vector<uint8_t> got(frame + 2 * guard, 0xaa), want(got);
    for (int b = 0; b < sub_h; b++)
      for (int a = 0; a < sub_w; a++)
        std::memcpy(want.data() + guard +
                        (((size_t)c.ystart + (size_t)b * c.yadd) * W + (size_t)c.xstart + (size_t)a * c.xadd) * 4,
                    &src[(size_t)b * sub_w + a], 4);
    sfrt::scatter_subset(src.data(), got.data() + guard, W, sub_w, sub_h, c.xstart, c.xadd, c.ystart,
                         c.yadd);
    EXPECT(got == want);
  }
}

static void check_cachebuf() {
  EXPECT(sfrt::grown_capacity(0, 0) == 256 && sfrt::grown_capacity(0, 256) == 256);
  EXPECT(sfrt::grown_capacity(0, 257) == 384 && sfrt::grown_capacity(384, 385) == 576);
  EXPECT(sfrt::grown_capacity(1000, 10) == 1000);
  for (size_t cap : {(size_t)0, (size_t)300, (size_t)1 << 20})
    for (size_t need : {(size_t)1, (size_t)5000, (size_t)3 << 20}) {
      const size_t c = sfrt::grown_capacity(cap, need);
      EXPECT(c >= need && c >= cap && c >= 256);
      EXPECT(c == (cap > 256 ? cap : 256) || c - c / 3 <= need + 1);  // the last step was needed
      EXPECT(sfrt::grown_capacity(cap, c) == c);  // asking for the capacity allocates exactly it
    }
  // geometric: every buffer a steadily growing owner retired, together, stays below twice its
  // live one (each is at most 2/3 of the next)
  size_t cap = 0, retired = 0;
  for (size_t need = 1000; need < 2000000; need += 1000) {
    const size_t c = sfrt::grown_capacity(cap, need);
    if (c != cap) retired += cap;
    cap = c;
  }
  EXPECT(retired < 2 * cap);

  int frees = 0, allocs = 0;
  bool fail_free = false, fail_alloc = false;
  const auto free_fn = [&](void* p) {
    if (fail_free) return false;
    std::free(p);
    frees++;
    return true;
  };
  const auto alloc_fn = [&](long long n) -> void* {
    if (fail_alloc) return nullptr;
    allocs++;
    return std::malloc((size_t)n);
  };
  CacheBuf b;
  EXPECT(!b.reserve(0, free_fn, alloc_fn) && !b.ptr && b.bytes == 0);
  EXPECT(b.reserve(100, free_fn, alloc_fn) && b.ptr && b.bytes == 100 && allocs == 1);
  void* p0 = b.ptr;
  EXPECT(b.reserve(60, free_fn, alloc_fn) && b.ptr == p0 && b.bytes == 100 && allocs == 1 && frees == 0);
  fail_free = true;  // the old buffer and its size stay: it is still the owner's to free
  EXPECT(!b.reserve(200, free_fn, alloc_fn) && b.ptr == p0 && b.bytes == 100 && allocs == 1);
  fail_free = false;
  fail_alloc = true;  // freed, then nothing: null and zero, never the freed pointer
  EXPECT(!b.reserve(200, free_fn, alloc_fn) && !b.ptr && b.bytes == 0 && frees == 1);
  fail_alloc = false;
  EXPECT(b.reserve(200, free_fn, alloc_fn) && b.ptr && b.bytes == 200 && allocs == 2 && frees == 1);
  b.release(free_fn);
  EXPECT(!b.ptr && b.bytes == 0 && frees == 2);
  b.release(free_fn);  // released twice: no second free
  EXPECT(frees == 2);
  const void* lo = (const void*)(uintptr_t)64;
  const void* odd = (const void*)(uintptr_t)66;
  EXPECT(sfrt::aligned4({lo, nullptr, lo}) && !sfrt::aligned4({lo, odd}) && sfrt::aligned4({}));
}

int main() {
  check_layouts();
  check_scatter();
  check_cachebuf();
  if (failures) return 1;
  std::printf("hostmem_check ok\n");
  return 0;
}
