// sfrt_hostmem.h -- the host layer's buffer bookkeeping and layouts, without a HIP call of their
// own ("Host memory"): the one growable buffer every owner in sfrt_host.h and
// sfrt_raycache.h is built on, the staging layout of a ray batch, the scatter of a compact subset
// into the caller's frame.  Tested on the host: tests/native/hostmem_check.cpp (and, for
// CacheBuf under a chain's caches, tests/native/tilerec_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace sfrt {

// The capacity a buffer of `cap` grows to for `need`: geometric (each buffer at most 2/3 of the
// next), so all its owner ever retired (RetiredHost) stays below twice what it holds.
inline size_t grown_capacity(size_t cap, size_t need) {
  size_t c = cap > 256 ? cap : 256;
  while (c < need) c += c / 2;
  return c;
}

// One grow-only buffer and its size: the caller passes how to free and how to allocate
// (sfrt_host.h DeviceBuf: stream-ordered; PinnedBuf: retire, hipHostMalloc; the tests: counters).
struct CacheBuf {
  void* ptr = nullptr;
  long long bytes = 0;

  // Room for `need` bytes: a buffer that is large enough stays (its contents too), a smaller
  // one is freed (free_fn(ptr) -> bool) and replaced (alloc_fn(need) -> pointer or null).  The
  // pointer is null and the size zero before the allocation, so a failed one leaves a consistent
  // object.  false: the buffer may be gone (bytes == 0) and nothing may be read from it.
  template <class Free, class Alloc>
  bool reserve(long long need, Free&& free_fn, Alloc&& alloc_fn) {
    if (need <= 0) return false;
    if (need <= bytes) return true;
    if (ptr && !free_fn(ptr)) return false;
    ptr = nullptr;
    bytes = 0;
    ptr = alloc_fn(need);
    if (!ptr) return false;
    bytes = need;
    return true;
  }
  template <class Free>
  void release(Free&& free_fn) {
    if (ptr) (void)free_fn(ptr);
    ptr = nullptr;
    bytes = 0;
  }
};

inline bool aligned4(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 3u) return false;
  return true;
}

// One array of a ray batch in the caller's memory: n elements of `elem` bytes, or absent (null).
struct BatchPart {
  const void* host;
  size_t elem;
};

// The staging layout of a batch of n rays: the present inputs back to back from offset 0, then
// the requested outputs; an absent array takes no room.  One H2D copy of [0, in_bytes) and one
// D2H copy of [in_bytes, bytes) move a whole batch.
struct BatchLayout {
  static constexpr int kMaxParts = 6;
  size_t n = 0, in_bytes = 0, bytes = 0;
  int n_in = 0, n_out = 0;
  BatchPart in[kMaxParts] = {}, out[kMaxParts] = {};
  size_t in_off[kMaxParts] = {}, out_off[kMaxParts] = {};

  BatchLayout(size_t count, std::initializer_list<BatchPart> inputs,
              std::initializer_list<BatchPart> outputs)
      : n(count) {
    for (const BatchPart& p : inputs) {
      in[n_in] = p;
      in_off[n_in++] = bytes;
      if (p.host) bytes += n * p.elem;
    }
    in_bytes = bytes;
    for (const BatchPart& p : outputs) {
      out[n_out] = p;
      out_off[n_out++] = bytes;
      if (p.host) bytes += n * p.elem;
    }
  }
  // Input / output q's place in a staging buffer at `base`, null when absent.
  template <class T>
  T* in_at(void* base, int q) const {
    return in[q].host ? (T*)((uint8_t*)base + in_off[q]) : nullptr;
  }
  template <class T>
  T* out_at(void* base, int q) const {
    return out[q].host ? (T*)((uint8_t*)base + out_off[q]) : nullptr;
  }
  // The caller's inputs into host staging; host staging's outputs to the caller, but for those
  // whose bit is set in `skip`.
  void stage_inputs(void* staging) const {
    for (int q = 0; q < n_in; q++)
      if (in[q].host) std::memcpy((uint8_t*)staging + in_off[q], in[q].host, n * in[q].elem);
  }
  void copy_outputs(const void* staging, unsigned skip = 0) const {
    for (int q = 0; q < n_out; q++)
      if (out[q].host && !((skip >> q) & 1u))
        std::memcpy((void*)out[q].host, (const uint8_t*)staging + out_off[q], n * out[q].elem);
  }
};

// A compact sub_w x sub_h subset (4-byte elements, row-major) into the caller's frame of `width`
// elements per row: element (a, b) goes to column xstart + a * xadd of row ystart + b * yadd.
// Only addressed elements are written.
inline void scatter_subset(const uint32_t* src, uint8_t* dst, size_t width, int sub_w, int sub_h,
                           int xstart, int xadd, int ystart, int yadd) {
  for (int b = 0; b < sub_h; b++) {
    const uint32_t* from = src + (size_t)b * sub_w;
    uint8_t* row = dst + (((size_t)ystart + (size_t)b * yadd) * width + (size_t)xstart) * 4;
    if (xadd == 1) {
      std::memcpy(row, from, (size_t)sub_w * 4);
    } else {
      for (int a = 0; a < sub_w; a++) std::memcpy(row + (size_t)a * xadd * 4, from + a, 4);
    }
  }
}

}  // namespace sfrt
