// sphere_trace.hip -- gfx950 kernels for the sphere-cave trace-and-shade path.
//
// Replaces the per-pixel body of SphereWorld::UpdateImage / Raycast
// (/root/reference/Raytracing/SphereWorld.cpp:83-112, 355-382): one wave64 per
// (8R)x8 pixel tile, R = 1..4 pixels per lane (records in the kernel arguments for
// n <= 64 spheres, a per-wave culled list above that), RGBA8 written straight to HBM.
//
// Bit-exactness rules (see DESIGN.md "Exactness"):
//  * built with -ffp-contract=off; every float expression keeps the
//    reference's operand order; division and sqrt are the correctly rounded
//    gfx950 sequences (hipcc default), or the same sequences without their
//    range scaling where the operands provably need none (div_inrange,
//    sqrt_cr_normal: sfrt_device.h);
//  * atan2f / asinf are sfrt_math:: restatements of the host libm;
//  * the sphere test `r - sqrtf(s) > 0.01f` is replaced by `s < s_pass`, where
//    s_pass is the exact binary32 threshold found on the host (the test is
//    monotone in s), so sqrtf runs only for spheres that pass;
//  * a sphere is skipped for a whole wave only when it provably cannot pass
//    for any ray of the tile (cone test with margins, below); the surviving
//    spheres are visited in their original order, so "last passing index"
//    (drawSphere, :368) and the max (:367) are unchanged.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "sfrt_device.h"
#include "sfrt_math.h"
#include "sfrt_probe.h"
#include "sfrt_raycache.h"
#include "sfrt_trace.h"

#pragma clang fp contract(off)

// Diagnostic builds (-DSFRT_EXP=<bits>: timing and counter probes that write wrong bytes) go
// through the probe type P of trace_tile_window_r (sfrt_probe.h); the shipped library's
// NoProbe hooks are empty.
#ifndef SFRT_BUILD_FLAVOUR
#define SFRT_BUILD_FLAVOUR "release"
#endif

namespace sfrt {
namespace {

constexpr float kPI = 3.1415926535f;     // SphereWorld.h:6
constexpr float kPI2 = 6.28318530718f;   // SphereWorld.h:7

// subset_index<SS> (compact subset index -> frame column or row) is in sfrt_device.h.
// The stride of the compact index as a float, for the tile centre of the culling cone (an
// axis only: the cone's half-angle is measured from the rays themselves).
template <int SS>
__device__ __forceinline__ float subset_stride(int add) {
  if constexpr (SS == 0) return (float)add;
  else return (float)add * (1.0f / (float)(1 << SS));
}

// Primary direction of pixel (i, j), normalised (SphereWorld.cpp:95-106, :358).
__device__ __forceinline__ void primary_dir(const FrameRec& f, int i, int j, float& dx,
                                            float& dy, float& dz) {
  const float h = f.h_start + f.h_inc * (float)i;
  const float v = f.v_start + (float)j * f.v_inc;
  float x = (f.fwd[0] + f.right[0] * h) + f.up[0] * v;
  float y = (f.fwd[1] + f.right[1] * h) + f.up[1] * v;
  float z = (f.fwd[2] + f.right[2] * h) + f.up[2] * v;
  // |(x,y,z)|^2 >= 1 - tiny: forward is a unit vector orthogonal to right and up
  const float len = sqrt_cr_normal((x * x + y * y) + z * z);
  // components in [2^-40, 2^40) put len there too: one shared reciprocal seed
  // (div_inrange, the same bits as `/`); a wave with a zero component takes `/`
  if ((ballot_bad_operand(x) | ballot_bad_operand(y) | ballot_bad_operand(z)) == 0) {
    const float s = div_seed(len);
    dx = div_inrange(x, len, s);
    dy = div_inrange(y, len, s);
    dz = div_inrange(z, len, s);
  } else {
    const float l = keep_branch(len);
    dx = x / l;
    dy = y / l;
    dz = z / l;
  }
}

// The ray cache (sfrt_raycache.h; DESIGN.md 5 "Ray cache"): the directions primary_dir gives a
// tile's rays, tile-major in the kernel's own tile / lane / slot mapping, clamped edge
// duplicates included -- [tile][component x, y, z][lane][r] binary32, so a wave reads (and
// k_ray_fill writes) three contiguous runs of 256 R bytes, R dwords per lane and component
// (R = 4: one 16-byte access, the buffer and every run being 16-byte aligned).
template <int R>
struct RaySlots {
  float v[R];
};
template <int R>
__device__ __forceinline__ size_t ray_cache_at(int tile, int component, int lane) {
  return ((size_t)tile * 3u + (size_t)component) * (size_t)(64 * R) + (size_t)(lane * R);
}
template <int R>
__device__ __forceinline__ void ray_cache_load(const float* __restrict__ rc, int tile, int lane,
                                               float (&dx)[R], float (&dy)[R], float (&dz)[R]) {
  typedef RaySlots<R> __attribute__((aligned(R == 4 ? 16 : R == 2 ? 8 : 4))) Slots;
  const Slots x = *(const Slots*)(rc + ray_cache_at<R>(tile, 0, lane));
  const Slots y = *(const Slots*)(rc + ray_cache_at<R>(tile, 1, lane));
  const Slots z = *(const Slots*)(rc + ray_cache_at<R>(tile, 2, lane));
#pragma unroll
  for (int r = 0; r < R; r++) {
    dx[r] = x.v[r];
    dy[r] = y.v[r];
    dz[r] = z.v[r];
  }
}
template <int R>
__device__ __forceinline__ void ray_cache_store(float* __restrict__ rc, int tile, int lane,
                                                const float (&dx)[R], const float (&dy)[R],
                                                const float (&dz)[R]) {
  typedef RaySlots<R> __attribute__((aligned(R == 4 ? 16 : R == 2 ? 8 : 4))) Slots;
  Slots x, y, z;
#pragma unroll
  for (int r = 0; r < R; r++) {
    x.v[r] = dx[r];
    y.v[r] = dy[r];
    z.v[r] = dz[r];
  }
  *(Slots*)(rc + ray_cache_at<R>(tile, 0, lane)) = x;
  *(Slots*)(rc + ray_cache_at<R>(tile, 1, lane)) = y;
  *(Slots*)(rc + ray_cache_at<R>(tile, 2, lane)) = z;
}

// The directions of tile `tile`'s rays as the march takes them: lane l holds columns
// (l & 7) + 8 r of tile row l >> 3, clamped to the subset (edge lanes trace a duplicate).
template <int R, int SS>
__device__ __forceinline__ void tile_dirs(const FrameRec& f, int tile_x, int tile_y, int lane,
                                          float (&dx)[R], float (&dy)[R], float (&dz)[R]) {
  const int b = f.sub_row0 + tile_y * kTile + (lane >> 3);
  const int b_end = f.sub_row0 + f.sub_rows;
  const int bc = b < b_end ? b : b_end - 1;
  const int j = subset_index<SS>(f.ystart, f.yadd, bc);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int a = tile_x * R * kTile + r * kTile + (lane & 7);
    const int ac = a < f.sub_w ? a : f.sub_w - 1;
    primary_dir(f, subset_index<SS>(f.xstart, f.xadd, ac), j, dx[r], dy[r], dz[r]);
  }
}

// Shading tail, SphereWorld.cpp:373-381, in two parts so that a lane's R pixels
// can issue their texel loads together: shade_texel computes the texel index --
// `tex` indexes f.tex (the sphere's first texel when the index falls outside the
// texture: the reference would read outside the image there; `outside` reports
// it) -- and the brightness; shade_rgba applies the brightness (RGBA8 packed, r
// in byte 0).
struct Shading {
  uint32_t tex;
  float brightness;
  bool outside;
  float depth;  // AUX only: |pos - cam| (:375's VLength, the operand of its std::max)
  float fu, fw;  // the coordinates' fractions before the texture's size (the hit cache's record)
};

// ORIGIN (the ray batches, k_cast_rays): the brightness is taken from the ray's own origin
// (ox, oy, oz) in place of f.cam, :375's cam.pos.
// Everything above the line that reads d.tex_wh depends only on the position, f.cam, the drawn
// record's cx, cy, cz, r and atan_c: on nothing CullKey does not hold.  It ends in three floats --
// fu and fw, the fractions of the texture coordinates before they meet the texture's size, and
// the brightness -- which the function returns beside the rest (dead, and removed, wherever they
// are unused) and which the hit cache stores (sfrt_raycache.h HitRec).  FRAC (the k_shade_hits
// kernels): (px, py, pz) are those three floats, loaded, and the function is its texture-
// dependent part only -- the same bits into the same remaining instructions.
template <class P, bool AUX = false, bool ORIGIN = false, bool FRAC = false>
__device__ __forceinline__ Shading shade_texel(const FrameRec& f, const SphereRec& d, float px,
                                               float py, float pz, PixelDump* dump, float ox = 0.0f,
                                               float oy = 0.0f, float oz = 0.0f) {
  static_assert(!FRAC || (!AUX && !ORIGIN), "the fractions carry neither depth nor origin");
  [[maybe_unused]] float xcoord = 0.0f, ycoord = 0.0f, bl = 0.0f;
  float fu, fw, brightness;
  if constexpr (FRAC) {
    fu = px;
    fw = py;
    brightness = pz;
  } else {
    float ang = d.atan_c - P::hit_atan2(pz, px);  // atan2f_wave == sfrt_math::atan2f (sfrt_device.h)
    ang = ang > kPI ? ang - kPI2 : (ang < -kPI ? ang + kPI2 : ang);
    xcoord = sfrt_math::div_pi2_plus_1(ang);  // == ang / PI2 + 1.0f
    const float ex = px - d.cx, ey = py - d.cy, ez = pz - d.cz;
    const float el = sqrt_cr((ex * ex + ey * ey) + ez * ez);
    const float bx = px - (ORIGIN ? ox : f.cam[0]), by = py - (ORIGIN ? oy : f.cam[1]),
                bz = pz - (ORIGIN ? oz : f.cam[2]);
    bl = sqrt_cr((bx * bx + by * by) + bz * bz);
    const float bd = bl < 3.0f ? 3.0f : bl;
    // ey / el and 3 / bd through div_inrange (same bits) unless some lane's operands
    // leave [2^-40, 2^40) (bd >= 3 needs only the upper bound)
    float ny;
    if ((ballot_bad_operand(ey) | ballot_bad_operand(el) | __builtin_amdgcn_ballot_w64(!(bd < 0x1.0p40f))) == 0) {
      ny = div_inrange(ey, el);
      brightness = div_inrange(3.0f, bd);
    } else {
      ny = ey / keep_branch(el);
      brightness = 3.0f / keep_branch(bd);
    }
    ycoord = sfrt_math::div_pi_plus_half(P::hit_asin(ny));  // == asinf / PI + 0.5f
  }
  // fmodf(v, 1.0f) == v - truncf(v) exactly for every binary32 v (NaN/inf -> NaN).
  // texsize of textures[0] (or of the sphere's extension slot), (float)(unsigned) as :376
  // (the statements in this order: the marching kernels' schedule follows it)
  const uint32_t tw = d.tex_wh & 0xffffu, th = d.tex_wh >> 16;
  if constexpr (!FRAC) {
    const float u = xcoord * 4.0f * d.r;
    fu = u - __builtin_truncf(u);
  }
  const float su = fu * (float)tw;
  if constexpr (!FRAC) {
    const float w = ycoord * 2.0f * d.r;
    fw = w - __builtin_truncf(w);
  }
  const float sw = fw * (float)th;
  // float -> unsigned: v_cvt_u32_f32 (NaN -> 0), as x86's cvttss2si for [0, 2^31).
  const uint32_t tx = __float2uint_rz(su), ty = __float2uint_rz(sw);
  // ty < th <= 0xffff (a fraction in [0, 1) times th, or 0 from NaN; radii are > 0, so no
  // negative fraction reaches -1 / th): the 24-bit multiply is the exact product
  const uint32_t idx = tx + __umul24(ty, tw);
  Shading sh;
  sh.outside = !(idx < tw * th);
  sh.tex = d.tex_off + (sh.outside ? 0u : idx);
  sh.brightness = brightness;
  sh.fu = fu;
  sh.fw = fw;
  if constexpr (AUX) sh.depth = bl;
  else sh.depth = 0.0f;
  if (dump) {
    dump->xcoord = xcoord;
    dump->ycoord = ycoord;
    dump->brightness = brightness;
    dump->texel[0] = tx;
    dump->texel[1] = ty;
  }
  return sh;
}

// (Uint8)(component * brightness) for r, g, b; alpha kept (:377-379, :109).
[[maybe_unused]] __device__ __forceinline__ uint32_t shade_rgba(uint32_t texel, float brightness) {
  const uint32_t r = __float2uint_rz((float)(texel & 0xffu) * brightness);
  const uint32_t g = __float2uint_rz((float)((texel >> 8) & 0xffu) * brightness);
  const uint32_t b = __float2uint_rz((float)((texel >> 16) & 0xffu) * brightness);
  return (r & 0xffu) | ((g & 0xffu) << 8) | ((b & 0xffu) << 16) | (texel & 0xff000000u);
}

// Cone of the wave's rays: unit axis through the tile centre, and the sine
// and cosine of a half-angle that contains every lane's unit ray.  The sine
// is taken from |d x a| (accurate for the small angles of a tile, unlike a
// cosine near 1), maximised over the wave, plus slack for binary32 rounding.
// A tile whose rays spread past ~60 degrees (strided subsets) gets wide = true
// and is not culled.
// Square roots of the culling geometry (cone, window): the raw v_sqrt_f32, within 1 ulp of
// the correctly rounded root for normal arguments (the compiler's sqrtf adds a rescaling for
// arguments below 2^-96 and a correction step).  Every use is covered by a slack far above
// 1 ulp: 4e-6 |w| on the cone distances, 1e-5 on the half-angle's sine and relative on the
// window half-width, plus the absolute cull margin; below 2^-96 the root's absolute error is
// below 2^-48 either way.
__device__ __forceinline__ float sqrt_cull(float x) { return __builtin_amdgcn_sqrtf(x); }

struct Cone {
  float ax, ay, az, cos_t, sin_t;
  bool wide;
};

// Wave-level cull ("wavefront ballot") plus march window.  Lane l tests sphere
// base + l against the cone; bit l of the result is set when the sphere may
// pass the march test for some ray of the wave's tile.  A sphere is dropped
// only when its distance to the cone exceeds its radius inflated by
// f.cull_margin, which bounds how far the binary32 march positions can drift
// from their rays (sfrt_world.cpp) -- there r - |p - c| > 0.01f cannot hold.
// The distance from a centre at axial coordinate t and radial distance perp to
// the cone's side line is perp * cos_t - t * sin_t; it is the distance to the
// cone where the centre projects onto the side, and a lower bound of it
// everywhere (behind the apex the distance is |w|).  Evaluating it in binary32
// errs by < 1e-6 |w|, covered by the 4e-6 |w| slack.  Spheres whose pass
// threshold is 0 never pass and are dropped.  In addition lane l returns, for
// sphere base + l, an interval (lo, hi) of along-ray distance outside which
// the sphere cannot pass for any ray of the cone.  A ray's march position p
// at along-ray distance tau lies within the drift bound of the ray's point
// cam + u*tau (cull_margin), so a pass needs |cam + u*tau - c| < rr, i.e.
// |tau - dot(w, u)| < sqrt(rr^2 - d^2) with d the distance of the centre from
// the ray's line (the half-width h below bounds it over the cone).  Over the
// cone's rays dot(w, u) = |w| cos(angle(w, u)) with the angle in
// [max(0, alpha - theta), min(pi, alpha + theta)] (alpha = angle(w, axis),
// theta = half-angle): |w| cos(alpha -+ theta) = t cos_t +- perp sin_t,
// clamped to +-|w| where alpha - theta < 0 or alpha + theta > pi.  The
// interval is widened by h + cull_margin: the binary32 error of the lanes'
// accumulated distance (<= 1.3e-4 R over kCullSafeIterations steps) and of
// these expressions fit in the second margin.
__device__ __forceinline__ uint64_t cull_window(const FrameRec& f, const SphereRec* __restrict__ sph,
                                                int base, const Cone& c, float& lo, float& hi) {
  const int k = base + (int)(threadIdx.x & 63);
  bool inc = false;
  lo = __builtin_inff();
  hi = -__builtin_inff();
  if (k < f.n) {
    const SphereRec s = sph[k];
    if (s.s_pass > 0.0f) {
      const float wx = s.cx - f.cam[0], wy = s.cy - f.cam[1], wz = s.cz - f.cam[2];
      const float wl = sqrt_cull((wx * wx + wy * wy) + wz * wz);
      const float rr = s.r + f.cull_margin + 4e-6f * wl;
      const float t = (wx * c.ax + wy * c.ay) + wz * c.az;
      const float px = wx - t * c.ax, py = wy - t * c.ay, pz = wz - t * c.az;
      const float perp = sqrt_cull((px * px + py * py) + pz * pz);
      const bool side = t * c.cos_t + perp * c.sin_t >= -rr;
      const float sa = perp * c.cos_t - t * c.sin_t;  // |w| sin(alpha - theta)
      inc = c.wide || wl <= rr || (side && sa <= rr);
      if (inc) {
        if (c.wide) {
          hi = __builtin_inff();
          lo = -__builtin_inff();
        } else {
          const float sb = perp * c.cos_t + t * c.sin_t;  // |w| sin(alpha + theta)
          const float up = sa >= 0.0f ? t * c.cos_t + perp * c.sin_t : wl;
          const float dn = sb >= 0.0f ? t * c.cos_t - perp * c.sin_t : -wl;
          // Half-width: a ray whose line passes the centre at distance d has |q - c|^2 =
          // (tau - dot(w, u))^2 + d^2 at its exact point q(tau), so a pass (|q - c| < rr)
          // needs |tau - dot(w, u)| < sqrt(rr^2 - d^2).  Over the cone d >= |w| *
          // min(sin(alpha - theta), sin(alpha + theta)) = min(sa, sb) when both are >= 0
          // (else the cone's angles reach 0 or pi and d can be 0), taken 4e-6 |w| lower
          // for the binary32 error of sa and sb; the product form keeps the root's
          // relative error at a few ulps, and the 1e-5 relative slack covers it.
          const float dmin = fmaxf(0.0f, fminf(sa, sb) - 4e-6f * wl);
          const float h = sqrt_cull((rr - dmin) * (rr + dmin)) * 1.00001f;
          const float ext = h + f.cull_margin;
          lo = dn - ext;
          hi = up + ext;
        }
      }
    }
  }
  return __builtin_amdgcn_ballot_w64(inc);
}

// Record k read through the constant address space: the records are never written
// while a launch runs (kernel arguments, or a device ring slot reused only after the
// event of the launch that read it), and wave-uniform loads from that space are scalar
// loads -- through the generic pointer the compiler must assume the frame's stores may
// alias them and emits vector loads into VGPRs (the n > 64 kernel's records).
// k is unsigned and < 2^27, so k * 32 is a 32-bit byte offset the scalar load takes as its
// SGPR offset (a signed index costs a 64-bit shift and add per record).
__device__ __forceinline__ SphereRec rec_at(const SphereRec* p, uint32_t k) {
  const __attribute__((address_space(4))) uint32_t* q =
      (const __attribute__((address_space(4))) uint32_t*)(
          (const __attribute__((address_space(4))) char*)p + k * (uint32_t)sizeof(SphereRec));
  uint32_t w[sizeof(SphereRec) / 4];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(SphereRec) / 4); i++) w[i] = q[i];
  SphereRec r;
  __builtin_memcpy(&r, w, sizeof r);
  return r;
}

// std::max(largestDist, t) (SphereWorld.cpp:367) for L >= +0 and t > 0.01f
// (the pass test), both finite: their bit patterns order like the values, so
// one v_max_u32 gives the compare-select's bits (v_max_f32 would first
// canonicalise the loop-carried L).
__device__ __forceinline__ float max_nonneg(float L, float t) {
  return __uint_as_float(__builtin_elementwise_max(__float_as_uint(L), __float_as_uint(t)));
}

// One sphere test of the march (SphereWorld.cpp:365-369), exact: the pass
// test is s < s_pass (see sfrt_world.cpp, pass_threshold) and sqrtf runs only
// for a sphere that passes.
__device__ __forceinline__ float dist2(float px, float py, float pz, float cx, float cy,
                                       float cz) {
  const float ex = px - cx, ey = py - cy, ez = pz - cz;
  return (ex * ex + ey * ey) + ez * ez;
}

// Cone of an (8R)x8 tile whose lanes hold R rays each (columns c, c + 8, ...).
template <int R, int SS = 0>
__device__ __forceinline__ Cone tile_cone_r(const FrameRec& f, int tile_x, int tile_y,
                                            const float (&dx)[R], const float (&dy)[R],
                                            const float (&dz)[R]) {
  const float ic = (float)f.xstart +
                   ((float)(tile_x * R * kTile) + (0.5f * (float)(R * kTile) - 0.5f)) * subset_stride<SS>(f.xadd);
  const float jc = (float)f.ystart +
                   ((float)(f.sub_row0 + tile_y * kTile) + 3.5f) * subset_stride<SS>(f.yadd);
  const float h = f.h_start + f.h_inc * ic;
  const float v = f.v_start + jc * f.v_inc;
  float ax = (f.fwd[0] + f.right[0] * h) + f.up[0] * v;
  float ay = (f.fwd[1] + f.right[1] * h) + f.up[1] * v;
  float az = (f.fwd[2] + f.right[2] * h) + f.up[2] * v;
  const float inv = __builtin_amdgcn_rsqf((ax * ax + ay * ay) + az * az);
  ax *= inv; ay *= inv; az *= inv;
  float sin_l = 0.0f;
  bool wide = false;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const float cx = dy[r] * az - dz[r] * ay, cy = dz[r] * ax - dx[r] * az,
                cz = dx[r] * ay - dy[r] * ax;
    sin_l = fmaxf(sin_l, sqrt_cull((cx * cx + cy * cy) + cz * cz));
    wide = wide || ((dx[r] * ax + dy[r] * ay) + dz[r] * az) < 0.5f;
  }
  Cone c;
  c.ax = ax; c.ay = ay; c.az = az;
  c.sin_t = fminf(1.0f, __uint_as_float(wave_max_u32(__float_as_uint(sin_l))) + 1e-5f);
  c.cos_t = sqrt_cull(fmaxf(0.0f, 1.0f - c.sin_t * c.sin_t));
  c.wide = __builtin_amdgcn_ballot_w64(wide) != 0;
  return c;
}


// The same cone from the tile's four corner rays only.  Restricted to the image plane
// {fwd + right h + up v}, the angle to the axis has convex sublevel sets below 90 degrees (a
// convex circular cone cut by a plane), so over the tile's rectangle of (h, v) it is largest
// at a corner; every ray of the tile, edge duplicates included, lies in that rectangle (h and
// v are monotone in the pixel indices, also after rounding).  So if every corner ray is
// within 60 degrees of the axis, so is every ray, and the largest corner sine plus the same
// 1e-5 slack bounds every ray's (the slack covers the binary32 error of the corners' and of
// the rays' directions, a few 1e-8); otherwise the tile is wide.  Lane l computes corner l % 4.
template <int R, int SS = 0>
__device__ __forceinline__ Cone tile_cone_corners(const FrameRec& f, int tile_x, int tile_y, int lane) {
  const float ic = (float)f.xstart +
                   ((float)(tile_x * R * kTile) + (0.5f * (float)(R * kTile) - 0.5f)) * subset_stride<SS>(f.xadd);
  const float jc = (float)f.ystart +
                   ((float)(f.sub_row0 + tile_y * kTile) + 3.5f) * subset_stride<SS>(f.yadd);
  const float hc = f.h_start + f.h_inc * ic;
  const float vc = f.v_start + jc * f.v_inc;
  float ax = (f.fwd[0] + f.right[0] * hc) + f.up[0] * vc;
  float ay = (f.fwd[1] + f.right[1] * hc) + f.up[1] * vc;
  float az = (f.fwd[2] + f.right[2] * hc) + f.up[2] * vc;
  const float inv = __builtin_amdgcn_rsqf((ax * ax + ay * ay) + az * az);
  ax *= inv; ay *= inv; az *= inv;
  // corner lane % 4: column 0 or 8R - 1, row 0 or 7 of the tile, clamped like the rays
  const int a0 = tile_x * R * kTile + ((lane & 1) ? R * kTile - 1 : 0);
  const int b0 = f.sub_row0 + tile_y * kTile + ((lane & 2) ? kTile - 1 : 0);
  const int a = a0 < f.sub_w ? a0 : f.sub_w - 1;
  const int b = b0 < f.sub_row0 + f.sub_rows ? b0 : f.sub_row0 + f.sub_rows - 1;
  const float h = f.h_start + f.h_inc * (float)subset_index<SS>(f.xstart, f.xadd, a);
  const float v = f.v_start + (float)subset_index<SS>(f.ystart, f.yadd, b) * f.v_inc;
  float x = (f.fwd[0] + f.right[0] * h) + f.up[0] * v;
  float y = (f.fwd[1] + f.right[1] * h) + f.up[1] * v;
  float z = (f.fwd[2] + f.right[2] * h) + f.up[2] * v;
  const float il = __builtin_amdgcn_rsqf((x * x + y * y) + z * z);
  x *= il; y *= il; z *= il;
  const float cx = y * az - z * ay, cy = z * ax - x * az, cz = x * ay - y * ax;
  const float sin_l = sqrt_cull((cx * cx + cy * cy) + cz * cz);
  Cone c;
  c.ax = ax; c.ay = ay; c.az = az;
  c.sin_t = fminf(1.0f, __uint_as_float(wave_max_u32(__float_as_uint(sin_l))) + 1e-5f);
  c.cos_t = sqrt_cull(fmaxf(0.0f, 1.0f - c.sin_t * c.sin_t));
  c.wide = __builtin_amdgcn_ballot_w64(!(((x * ax + y * ay) + z * az) >= 0.5f)) != 0;
  return c;
}

// The tile's cone as the trace kernels and k_ray_fill both take it.
// R >= 3: four corner rays per wave are cheaper than R rays per lane (profiles/ab/r3_ab9)
template <int R, int SS>
__device__ __forceinline__ Cone tile_cone(const FrameRec& f, int tile_x, int tile_y, int lane,
                                          const float (&dx)[R], const float (&dy)[R],
                                          const float (&dz)[R]) {
  if constexpr (R >= 3) return tile_cone_corners<R, SS>(f, tile_x, tile_y, lane);
  else return tile_cone_r<R, SS>(f, tile_x, tile_y, dx, dy, dz);
}

// The tile records (sfrt_raycache.h TileRec; DESIGN.md 5 "Ray cache"): tile_cone's result and
// the tile's grid position, which depend on nothing outside the launch's RayKey.  Written by
// lane 0 of k_ray_fill's wave (plain vector stores); read like a sphere record (rec_at): the
// buffer is written only by the fill kernel that precedes the launch on its stream, never
// while a launch runs, so a wave-uniform load through the constant address space is one
// scalar 8-dword load.  The byte offset is 64-bit: an ordered grid has up to 2^28 tiles.
__device__ __forceinline__ void tile_rec_store(TileRec* __restrict__ tr, int tile, int tile_x,
                                               int tile_y, const Cone& c) {
  TileRec t;
  t.ax = c.ax; t.ay = c.ay; t.az = c.az;
  t.sin_t = c.sin_t; t.cos_t = c.cos_t;
  t.wide = c.wide ? 1u : 0u;
  t.tile_x = (uint32_t)tile_x; t.tile_y = (uint32_t)tile_y;
  tr[tile] = t;
}
__device__ __forceinline__ TileRec tile_rec_at(const TileRec* p, int tile) {
  const __attribute__((address_space(4))) uint32_t* q =
      (const __attribute__((address_space(4))) uint32_t*)(
          (const __attribute__((address_space(4))) char*)p + (size_t)tile * sizeof(TileRec));
  uint32_t w[sizeof(TileRec) / 4];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(TileRec) / 4); i++) w[i] = q[i];
  TileRec r;
  __builtin_memcpy(&r, w, sizeof r);
  return r;
}

// The cull cache (sfrt_raycache.h CullRec, CullWin, CullWinList; DESIGN.md 5 "Cull cache"): what
// cull_wave leaves a tile's wave, stored by k_cull_fill (plain vector stores, the record from
// lane 0) and loaded by the _cc kernels -- the record like a tile record (one scalar 4-dword
// load: the buffer is written only by the fill that precedes the launch on its stream), the
// lane's windows with one vector load of 8 (n > 64: 12) bytes.
template <bool LIST>
using CullLane = std::conditional_t<LIST, CullWinList, CullWin>;
__device__ __forceinline__ CullRec cull_rec_at(const CullRec* p, int tile) {
  const __attribute__((address_space(4))) uint32_t* q =
      (const __attribute__((address_space(4))) uint32_t*)(
          (const __attribute__((address_space(4))) char*)p + (size_t)tile * sizeof(CullRec));
  uint32_t w[sizeof(CullRec) / 4];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(CullRec) / 4); i++) w[i] = q[i];
  CullRec r;
  __builtin_memcpy(&r, w, sizeof r);
  return r;
}
__device__ __forceinline__ size_t cull_win_at(int tile, int lane) {
  return (size_t)tile * 64u + (size_t)lane;
}

// The hit cache (sfrt_raycache.h HitRec; DESIGN.md 5 "Hit cache"): what the march and the part of
// the shading tail that no texture enters leave a tile's rays, [tile][r][lane]: the two texture
// fractions and the brightness (shade_texel), drawSphere and the moving bit.  Stored by the _hf
// kernels from their shading tail (plain vector stores, one 16-byte store per ray slot: 1 KiB
// contiguous per wave) and loaded by the k_shade_hits kernels, R loads back to back.  The buffer
// is written only by the _hf launch that precedes the reading launches on its stream.
// hw: hit_pack_draw of the ray's drawSphere and of whether it still moved, taken after march_wave.
template <int R>
__device__ __forceinline__ void hit_store(HitRec* __restrict__ hr, int tile, int lane,
                                          const Shading (&sh)[R], const uint32_t (&hw)[R]) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    uint4 v;
    v.x = __float_as_uint(sh[r].fu);
    v.y = __float_as_uint(sh[r].fw);
    v.z = __float_as_uint(sh[r].brightness);
    v.w = hw[r];
    *(uint4*)(hr + hit_rec_at(tile, R, r, lane)) = v;
  }
}
// Returns whether some ray of the lane still moved at the guard.
template <int R>
__device__ __forceinline__ bool hit_load(const HitRec* __restrict__ hr, int tile, int lane,
                                         float (&fu)[R], float (&fw)[R], float (&br)[R],
                                         int (&draw)[R]) {
  uint4 v[R];
#pragma unroll
  for (int r = 0; r < R; r++) v[r] = *(const uint4*)(hr + hit_rec_at(tile, R, r, lane));
  bool moving = false;
#pragma unroll
  for (int r = 0; r < R; r++) {
    fu[r] = __uint_as_float(v[r].x);
    fw[r] = __uint_as_float(v[r].y);
    br[r] = __uint_as_float(v[r].z);
    draw[r] = hit_draw(v[r].w);
    moving = moving || hit_moving(v[r].w);
  }
  return moving;
}

// The texel cache (sfrt_raycache.h TexelRec; DESIGN.md 5 "Texel cache"): what shade_texel leaves a
// ray once the drawn record's texture offset and size have entered -- the texel's index in the
// atlas (or the sentinel: outside) and the brightness with the moving bit in its sign --
// [tile][r][lane] like the hit records.  Stored by the _tf kernels (k_shade_hits that run once per
// TexKey; one 8-byte store per ray slot, 512 B contiguous per wave), loaded by k_shade_texels.
// hit_load_w: hit_load with each record's fourth dword as stored, the moving bit per ray.
template <int R>
__device__ __forceinline__ bool hit_load_w(const HitRec* __restrict__ hr, int tile, int lane,
                                           float (&fu)[R], float (&fw)[R], float (&br)[R],
                                           int (&draw)[R], uint32_t (&w)[R]) {
  uint4 v[R];
#pragma unroll
  for (int r = 0; r < R; r++) v[r] = *(const uint4*)(hr + hit_rec_at(tile, R, r, lane));
  bool moving = false;
#pragma unroll
  for (int r = 0; r < R; r++) {
    fu[r] = __uint_as_float(v[r].x);
    fw[r] = __uint_as_float(v[r].y);
    br[r] = __uint_as_float(v[r].z);
    draw[r] = hit_draw(v[r].w);
    w[r] = v[r].w;
    moving = moving || hit_moving(v[r].w);
  }
  return moving;
}
template <int R>
__device__ __forceinline__ void texel_store(TexelRec* __restrict__ xr, int tile, int lane,
                                            const Shading (&sh)[R], const uint32_t (&hw)[R]) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    uint2 v;
    v.x = texel_pack_tex(sh[r].tex, sh[r].outside);
    v.y = texel_pack_bright(__float_as_uint(sh[r].brightness), hit_moving(hw[r]));
    *(uint2*)(xr + hit_rec_at(tile, R, r, lane)) = v;
  }
}
// tex: the records' first dwords as stored (the sentinel included); br: the brightness, bit 31
// cleared.  Returns whether some ray of the lane still moved at the guard.
template <int R>
__device__ __forceinline__ bool texel_load(const TexelRec* __restrict__ xr, int tile, int lane,
                                           int (&tex)[R], float (&br)[R]) {
  uint2 v[R];
#pragma unroll
  for (int r = 0; r < R; r++) v[r] = *(const uint2*)(xr + hit_rec_at(tile, R, r, lane));
  bool moving = false;
#pragma unroll
  for (int r = 0; r < R; r++) {
    tex[r] = (int)v[r].x;
    br[r] = __uint_as_float(texel_bright_bits(v[r].y));
    moving = moving || texel_moving(v[r].y);
  }
  return moving;
}

// The compact layer (sfrt_raycache.h CompactRec; DESIGN.md 5 "Compact layer"): a texel record in
// one dword, [tile][lane][r] in the lane map of k_shade_compact, whose lane owns R consecutive
// pixels of one row.  Stored once per TexKey by k_shade_texels_cf, a k_shade_texels whose lane
// (row, i) holds columns r * 8 + i: column c of a row belongs to the reader's lane row * 8 + c / R,
// slot c % R -- a bijection of the tile's 64 R slots, clamped duplicates included, so every record
// the reader loads was written.  The class comes from the table's own thresholds (bright_class_of:
// integer compares, fifteen steps a ray).
// mw: the texel records' second dwords as stored (the moving bit per ray).
template <int R>
__device__ __forceinline__ void compact_store(CompactRec* __restrict__ cr, int tile, int lane,
                                              const Shading (&sh)[R], const uint32_t (&mw)[R],
                                              const uint32_t* __restrict__ rep, uint32_t classes) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int c = r * kTile + (lane & 7);
    const uint32_t cls = bright_class_of(rep, classes, texel_bright_bits(__float_as_uint(sh[r].brightness)));
    cr[compact_rec_at(tile, R, (lane & ~7) + c / R, c % R)].w =
        compact_pack(sh[r].tex, sh[r].outside, cls, texel_moving(mw[r]));
  }
}
// texel_load with each record's second dword as stored.
template <int R>
__device__ __forceinline__ bool texel_load_w(const TexelRec* __restrict__ xr, int tile, int lane,
                                             int (&tex)[R], float (&br)[R], uint32_t (&w)[R]) {
  uint2 v[R];
#pragma unroll
  for (int r = 0; r < R; r++) v[r] = *(const uint2*)(xr + hit_rec_at(tile, R, r, lane));
  bool moving = false;
#pragma unroll
  for (int r = 0; r < R; r++) {
    tex[r] = (int)v[r].x;
    br[r] = __uint_as_float(texel_bright_bits(v[r].y));
    w[r] = v[r].y;
    moving = moving || texel_moving(v[r].y);
  }
  return moving;
}

// L = +0 for a lane's R rays at the start of a march step, two registers per
// v_mov_b64 (left to itself the compiler copies one zero register into three
// others and then pairs them: five moves a step for R = 4, not two).
template <int R>
__device__ __forceinline__ void zero_steps(float (&L)[R]) {
#pragma unroll
  for (int r = 0; r + 1 < R; r += 2) {
    uint64_t z;
    __asm__ volatile("v_mov_b64 %0, 0" : "=v"(z));
    L[r] = __uint_as_float((uint32_t)z);
    L[r + 1] = __uint_as_float((uint32_t)(z >> 32));
  }
  if (R & 1) L[R - 1] = 0.0f;
}

// Pass bodies of one sphere for the lane's R rays under one scalar branch.
// (Lane-masked selects through inline asm instead of these exec-masked
// updates were measured slower: 1% at R = 2, 15% at R = 1.)
// sqrt_cr_normal serves every passing lane, also ss < 2^-96, where it is not
// the correctly rounded sqrt: a pass needs rad - sqrtf(ss) > 0.01f, so
// rad > 2^-7, and rad - q == rad for any q < 2^-33, which both roots of such
// ss are (tests/native/wave_check.hip, every ss).
template <int R>
__device__ __forceinline__ bool pass_body_r(const float (&ss)[R], float s_pass, float rad, int k,
                                            float (&L)[R], int (&draw)[R]) {
  uint64_t any = 0;
#pragma unroll
  for (int r = 0; r < R; r++) any |= __builtin_amdgcn_ballot_w64(ss[r] < s_pass);
  if (any) {
    __asm__ volatile("; sphere passes for some ray of the wave");  // keeps the branch
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (ss[r] < s_pass) {
        const float t = rad - sqrt_cr_normal(ss[r]);
        L[r] = max_nonneg(L[r], t);
        draw[r] = k;
      }
    }
  }
  return any != 0;
}

// The march (SphereWorld.cpp:359-372) of one wave, shared by the frame kernels (one wave per
// (8R)x8 tile: trace_tile_window_r) and the ray batches (one wave per 64 rays, R = 1:
// cast_rays_wave).  Lane l holds R rays (a tile's columns c, c + 8, ...), so the
// wave-uniform half of a sphere visit --
// record load, window bits, branch -- is shared by R rays and each lane carries
// R independent dependency chains.  Per wave: cull the spheres against the cone of
// the wave's rays (cull_wave).  With n <= 64 (LIST = false, records in the kernel
// arguments) lane l holds sphere l's march window and bit l of the culling mask
// is sphere l; with n > 64 (LIST, records in device memory) the culled spheres
// of every 64-sphere word are compacted, in index order, into lanes 0.. of a
// culled list (cidx = the sphere index) -- a wave that culls more than 64
// visits every sphere every step instead (exact; rare at the tile sizes used).
// A wave with <= kSlots culled spheres holds them in SGPRs and tests each every
// step; otherwise each step visits, in index order, the culled spheres whose
// march window meets the along-ray distances [min over marching rays, max over
// the wave] (the low end refreshed every second step: it only rises).  The caller
// then shades and stores.
//
// A stopped ray advances unmasked: it had no passing sphere at its position
// (its last step visited every sphere that could pass for it) and never moves
// again, so each later step again has none: L = +0, draw unchanged, tacc + 0 =
// tacc, and p + d * (+0) = p -- also for p = -0, which a marching wave's ray
// only reaches through -0 + d * l0 with d of negative sign, so d * (+0) = -0.
//
// cull_wave: the cull against `cone`, which must contain every ray of the wave.  It leaves the
// culled spheres in m (LIST: culled-list entries), their windows in lo / hi and, LIST, entry
// `lane`'s sphere in cidx -- or clears `culled`: every step then visits every sphere.
template <bool LIST>
__device__ __forceinline__ void cull_wave(const FrameRec& f, const SphereRec* sph,
                                          const Cone& cone, int lane, bool& culled, uint64_t& m,
                                          float& lo, float& hi, int& cidx) {
  if (!LIST) {
    m = cull_window(f, sph, 0, cone, lo, hi);
  } else {
    __shared__ float s_list[3][64];  // compaction scratch: lo, hi, index
    int count = 0;
    const int nwords = (f.n + 63) >> 6;
    for (int w = 0; w < nwords; w++) {
      float wlo, whi;
      const uint64_t mw = cull_window(f, sph, w * 64, cone, wlo, whi);
      const int cw = __builtin_popcountll(mw);
      if (count + cw > 64) {
        culled = false;
        break;
      }
      if ((mw >> lane) & 1ull) {
        const int dst = count + (int)__builtin_amdgcn_mbcnt_hi(
                                    (uint32_t)(mw >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mw, 0u));
        s_list[0][dst] = wlo;
        s_list[1][dst] = whi;
        s_list[2][dst] = __int_as_float(w * 64 + lane);
      }
      count += cw;
    }
    __syncthreads();  // one wave: orders its own LDS writes before the reads
    if (culled) {
      m = count >= 64 ? ~0ull : ((1ull << count) - 1ull);
      if (lane < count) {
        lo = s_list[0][lane];
        hi = s_list[1][lane];
        cidx = __float_as_int(s_list[2][lane]);
      }
    }
  }
}

// A wave's rays as the march carries them, R per lane: the last passing sphere (drawSphere), the
// steps taken (the loop trips of :362; counted only where asked), the unit direction, the
// position, mv -- the last step length: > 0 while the ray marches, +0 once it stopped (`mv > 0`
// is one compare per step, where a loop-carried bool would be rematerialised through VGPRs) --
// and tacc, the along-ray distance marched (the binary32 sum of the steps).
template <int R>
struct Rays {
  int draw[R], iters[R];
  float dx[R], dy[R], dz[R], px[R], py[R], pz[R], mv[R], tacc[R];
  int trips = 0;  // output only, set by march_wave: the wave's loop trips, the host's first included
};

// march_wave: the steps, from the rays' state after the host's first trip (or before any: the
// batches' own origins) to every ray stopped or kMaxIterations trips, which sets status bit 1.
// The rays go in and come back by value, so that the loops run on locals of this function: it is
// optimised on its own before it is inlined, and through references the arrays would stay in
// memory form until then (more registers in every frame kernel).
// COUNT: iters counts each ray's steps.  P: the probe hooks (sfrt_probe.h).
template <int R, bool LIST, bool COUNT, class P>
__device__ __forceinline__ Rays<R> march_wave(const FrameRec& f, const SphereRec* sph, int lane, P& probe,
                                              bool culled, uint64_t m, float lo, float hi, int cidx,
                                              Rays<R> ray) {
  auto any_marching = [&]() {
    uint64_t q = 0;
#pragma unroll
    for (int r = 0; r < R; r++) q |= __builtin_amdgcn_ballot_w64(ray.mv[r] > 0.0f);
    return q != 0;
  };
  // sphere of culled entry e (wave-uniform)
  auto entry = [&](uint32_t e) { return LIST ? (uint32_t)__builtin_amdgcn_readlane(cidx, (int)e) : e; };
  // First set bit of a 64-bit culling mask, 63 for an empty mask (s_ff1 gives -1): entry 63 is
  // always readable -- a record of the n <= 64 kernel's argument block, or lane 63 of the list
  // (its sphere, or sphere 63 < n) -- so a lookahead past the last entry loads a record it never uses.
  static_assert(kInlineSpheres == 64,
                "entry 63 must be readable: record 63 of the 64-entry argument block, or lane 63 "
                "of the list kernel's culled list (that kernel runs only for n > kInlineSpheres, "
                "so lane 63's default sphere 63 exists)");
  auto first_entry = [](uint64_t x) -> uint32_t {
    uint32_t e;
    __asm__("s_ff1_i32_b64 %0, %1" : "=s"(e) : "s"(x));
    return e & 63u;
  };
  auto clear_entry = [](uint64_t x, uint32_t e) -> uint64_t { return x & ~(1ull << e); };  // s_bitset0

  // pos += dir * L (SphereWorld.cpp:371) on every lane (see above)
  auto advance = [&](const float (&L)[R]) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      ray.px[r] = ray.px[r] + ray.dx[r] * L[r];
      ray.py[r] = ray.py[r] + ray.dy[r] * L[r];
      ray.pz[r] = ray.pz[r] + ray.dz[r] * L[r];
      if constexpr (COUNT) ray.iters[r] += ray.mv[r] > 0.0f ? 1 : 0;  // a step of a marching ray
      ray.mv[r] = L[r];
      ray.tacc[r] = ray.tacc[r] + L[r];
    }
  };
  auto visit = [&](float cx, float cy, float cz, float rad, float s_pass, int k, float (&L)[R]) {
    float ss[R];
#pragma unroll
    for (int r = 0; r < R; r++) ss[r] = dist2(ray.px[r], ray.py[r], ray.pz[r], cx, cy, cz);
    probe.visit(pass_body_r<R>(ss, s_pass, rad, k, L, ray.draw));
  };
  // Every sphere in index order (no culling: cull off, or past kCullSafeIterations steps).
  auto visit_all = [&](float (&L)[R]) {
    for (int k = 0; k < f.n; k++) {
      const SphereRec s = rec_at(sph, k);
      visit(s.cx, s.cy, s.cz, s.r, s.s_pass, k, L);
    }
  };
  int trips = 1;
  // Culled steps run while trips < kCullSafeIterations (the margins' bound, sec. 4 of
  // DESIGN.md); a wave still marching then continues in the full-list loop below.  Each
  // loop is single-exit (the guard is its condition) with one body shape: a second exit,
  // or a full/culled branch inside the step, makes the compiler copy every loop-carried
  // register (draw, L) between register sets each step.
  const int cull_end = culled ? kCullSafeIterations : 1;
  if (kSlots > 0 && culled && __builtin_popcountll(m) <= kSlots) {
    constexpr int NS = kSlots > 0 ? kSlots : 1;
    // Few culled spheres: hold them in SGPR slots and test every one each step
    // (cheaper than maintaining the window).  Empty slots never pass.
    float scx[NS], scy[NS], scz[NS], sr[NS], ssp[NS];
    int sk[NS];
    uint64_t mm = m;
#pragma unroll
    for (int q = 0; q < kSlots; q++) {
      scx[q] = scy[q] = scz[q] = sr[q] = ssp[q] = 0.0f;
      sk[q] = 0;
      if (mm) {
        const int k = entry(__builtin_ctzll(mm));
        mm &= mm - 1;
        const SphereRec s = rec_at(sph, k);
        scx[q] = s.cx; scy[q] = s.cy; scz[q] = s.cz;
        sr[q] = s.r; ssp[q] = s.s_pass;
        sk[q] = k;
      }
    }
    for (; any_marching() && trips < cull_end; ++trips) {
      float L[R];
      zero_steps<R>(L);
#pragma unroll
      for (int q = 0; q < kSlots; q++) visit(scx[q], scy[q], scz[q], sr[q], ssp[q], sk[q], L);
      advance(L);
    }
  } else {
    probe.window_mode();
    float tlo = 0.0f;
    for (; any_marching() && trips < cull_end; ++trips) {
      float L[R];
      zero_steps<R>(L);
      // tacc >= +0: reduce the bit patterns (wave_min_u32 / wave_max_u32)
      uint32_t th = 0u;  // +0
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t u = __float_as_uint(ray.tacc[r]);
        th = u > th ? u : th;
      }
      if (trips % 2 == 1) {  // the low end, every second step (every 3rd/4th: slower)
        uint32_t tl = 0x7f800000u;  // +inf
        if constexpr (R == 1) {  // the one ray's own value: the minimum with +inf costs a v_min_u32
          tl = ray.mv[0] > 0.0f ? __float_as_uint(ray.tacc[0]) : tl;
        } else {
#pragma unroll
          for (int r = 0; r < R; r++) {
            const uint32_t u = __float_as_uint(ray.tacc[r]);
            const uint32_t ua = ray.mv[r] > 0.0f ? u : 0x7f800000u;
            tl = ua < tl ? ua : tl;
          }
        }
        tlo = __uint_as_float(wave_min_u32(tl));
      }
      const float thi = __uint_as_float(wave_max_u32(th));
      const uint64_t win =
          m & __builtin_amdgcn_ballot_w64(lo < thi) & __builtin_amdgcn_ballot_w64(hi > tlo);
      // The visits, in index order, each issuing the next record's scalar loads
      // before its own arithmetic (the loads' latency hides under the R rays'
      // distance tests; past the last entry the lookahead loads entry 63's record,
      // unused).  Scalar work per visit is kept short: the scalar unit is shared by
      // the CU's four SIMDs (profiles/r3y_salu_mix_check.txt).
      if (win) {
        uint32_t e = first_entry(win);
        uint64_t mm = clear_entry(win, e);
        uint32_t k = entry(e);
        const SphereRec s0 = rec_at(sph, k);
        float cx = s0.cx, cy = s0.cy, cz = s0.cz, rad = s0.r, sp = s0.s_pass;
        bool more;
        do {  // the exit test at the bottom: a mid-loop exit made the back edge ~18 scalar ops
          const uint32_t en = first_entry(mm);
          const uint32_t kn = entry(en);
          const SphereRec sn = rec_at(sph, kn);
          const float ncx = sn.cx, ncy = sn.cy, ncz = sn.cz, nr = sn.r, nsp = sn.s_pass;
          visit(cx, cy, cz, rad, sp, (int)k, L);
          more = mm != 0;
          mm = clear_entry(mm, en);
          k = kn; cx = ncx; cy = ncy; cz = ncz; rad = nr; sp = nsp;
        } while (more);
      }
      advance(L);
    }
  }
  // Every sphere in index order, every step: culling off, or past kCullSafeIterations.
  for (; any_marching() && trips < kMaxIterations; ++trips) {
    float L[R];
    zero_steps<R>(L);
    visit_all(L);
    advance(L);
  }
  if (trips >= kMaxIterations && any_marching() && lane == 0) atomicOr(f.status, 1);
  ray.trips = trips;
  return ray;
}

// The frame fill: one wave per (8R)x8 tile sets its rays up, culls against the tile's cone,
// marches (march_wave), shades and stores.
// Edge lanes trace a clamped duplicate pixel (never stored) as the duplicate
// it is, which keeps the tile cone tight.
// DUMP (sfrt_world_trace_points only): the same march and shading, plus a per-ray
// iteration count and an epilogue writing the float intermediates of listed pixels.
// P: the probe hooks (sfrt_probe.h; NoProbe in the shipped library, all empty).
// SS (SFRT_OPT_SUPERSAMPLE, S = 1 << SS = 2 or 4): the tile is of sample pixels -- the
// pixels of the S*width x S*height frame (FrameRec) -- cull, march and shading as for any
// frame; the epilogue then box-filters each S x S group of samples, which sits in S x S
// lanes of the wave (sfrt_device.h group_sum_u32), into the one output pixel its leader lane
// stores.  S divides the tile's 8 rows and 8-column slots, and the subset's width and rows
// are multiples of S, so a group is wholly inside the subset or wholly clamped duplicates.
// CACHED: the rays' directions are loaded from the chain's ray cache rc (filled by k_ray_fill
// for this launch's RayKey: the bits primary_dir gives) and not computed, and the tile's cone
// and grid position from the chain's tile records tr (the bits tile_cone gives); all else is
// the same.
// AUX (sfrt_world_render_band_aux): the same march, shading and colour store,
// plus the per-ray step count of DUMP and, beside each colour store and under its condition,
// one dword per non-null plane of `aux` (sfrt_trace.h AuxArgs): the hit distance shade_texel
// computes for the brightness, drawSphere and the step count.  Supersampled, the leader lane
// stores its own sample's values (the group's first sample), unfiltered.
// CULLED (implies CACHED): the tile's culling mask, the lane's march window (and list entry) and
// the tile's grid position are loaded from the chain's cull cache cr / cw (filled by k_cull_fill
// for this launch's CullKey: the bits cull_wave gives) -- neither the tile record nor the sphere
// records are read before the march.
// HIT (implies CULLED; DESIGN.md 5 "Hit cache"): 1, the _hf kernels -- the CULLED launch, which
// also stores, from its shading tail, each ray's record in the chain's hit cache hr (hit_store):
// the fractions and the brightness shade_texel has before the texture's size enters, drawSphere
// and the moving bit, the bits the very same march and tail under the very same flags leave;
// 2, the k_shade_hits kernels -- one wave per tile in tile-number order (the grid is exactly the
// tiles: no sorter workgroup, no order lookup, no cost store), the tile's grid position from its
// CullRec, the rays' records loaded from hr in place of the ray setup, the cull, the march and
// the texture-independent part of the tail, of the drawn records only tex_off and tex_wh, then
// the rest of the same tail (shade_texel's FRAC): it is this function's, so there is one copy of
// it and the marching kernels' code cannot move when the reading kernels change.  A ray that
// still moved at the guard raises status bit 0 again;
// 3, the _tf kernels (DESIGN.md 5 "Texel cache") -- 2, which also stores, after shade_texel, each
// lane's texel record in the chain's texel cache xr (texel_store): the texel's index in the atlas
// or the sentinel, and the brightness with the record's moving bit in its sign;
// 4, k_shade_texels -- 2 with the rays' texel records loaded from xr in place of the hit records:
// no SphereRec is read and shade_texel is not entered, the index is the one it left; then the
// same texel loads, shade_rgba, box filter and stores.  Status bit 0 comes from the moving bits,
// bit 2 from the sentinel of a valid lane.
// CF (with HIT 4, SS 0; DESIGN.md 5 "Compact layer"): k_shade_texels_cf -- 4, which also stores each
// ray's compact record in cf (compact_store), in the lane map of k_shade_compact, the kernel that
// reads them and is no instantiation of this function.
// PLACE (sfrt_world_render_subset): the subset goes in place into a whole frame --
// compact column a (output pixel a >> SS) is stored xstride elements apart, the host having put
// the subset's first pixel into f.out and yadd frame rows into f.out_pitch (the planes' pitches
// likewise) -- where every other launch stores it compactly.  All else is the same.
template <int R, bool LIST, bool DUMP, class P, int SS = 0, bool CACHED = false, bool AUX = false,
          bool PLACE = false, bool CULLED = false, int HIT = 0, bool CF = false>
__device__ __forceinline__ void trace_tile_window_r(const FrameRec& f,
                                                    const SphereRec* __restrict__ sph,
                                                    DumpArgs dmp,
                                                    const float* __restrict__ rc = nullptr,
                                                    const TileRec* tr = nullptr,
                                                    AuxArgs aux = AuxArgs{},
                                                    [[maybe_unused]] int xstride = 1,
                                                    [[maybe_unused]] const CullRec* cr = nullptr,
                                                    [[maybe_unused]] const CullLane<LIST>* cw = nullptr,
                                                    [[maybe_unused]] HitRec* hr = nullptr,
                                                    [[maybe_unused]] TexelRec* xr = nullptr,
                                                    [[maybe_unused]] CompactRec* cf = nullptr,
                                                    [[maybe_unused]] const uint32_t* rep = nullptr,
                                                    [[maybe_unused]] uint32_t classes = 0) {
  // the launches that march nothing: 2 and 3 shade from the hit records, 4 from the texel records
  constexpr bool READS = HIT >= 2;
  static_assert(HIT >= 0 && HIT <= 4, "0, _hf, k_shade_hits, _tf, k_shade_texels");
  static_assert(!CF || (HIT == 4 && SS == 0), "k_shade_texels_cf: the compact fill rides on a texel read");
  static_assert(!CULLED || CACHED, "the cull cache rides on the ray cache");
  static_assert(HIT == 0 || (CULLED && !DUMP && !AUX && !PLACE), "the hit cache rides on the cull cache");
  static_assert(!PLACE || (!DUMP && !CACHED), "the placing kernels compute their directions and dump nothing");
  static_assert(SS == 0 || !DUMP, "trace_points dumps the 1x pixel");
  static_assert(!CACHED || !DUMP, "the DUMP kernels compute their directions");
  static_assert(!AUX || (!DUMP && !CACHED), "the AUX kernels compute their directions and dump nothing");
  const int lane = threadIdx.x & 63;
  P probe;
  probe.wave_entry();
  // Adaptive tile order (sfrt_trace.h FrameRec): workgroup 0 may be the sorter.
  const int ntiles = f.tiles_x * ((f.sub_rows + kTile - 1) / kTile);
  int slot = (int)blockIdx.x;
  if constexpr (!READS) {
    if (f.prev_cost) {
      if (blockIdx.x == 0) {
        sort_tiles(f.prev_cost, ntiles, f.next_order, f.order_dilate != 0);
        return;
      }
      slot -= 1;
    }
  }
  [[maybe_unused]] uint32_t cls;  // the tile's class in the order (sfrt_device.h slot_tile)
  const int tile = READS ? slot : slot_tile(f.tile_order, slot, ntiles, cls);
  int tile_x, tile_y;
  [[maybe_unused]] TileRec trec;
  [[maybe_unused]] CullRec crec;
  [[maybe_unused]] CullLane<LIST> cwin;
  if constexpr (CULLED) {
    if (tile >= ntiles) return;  // as below
    crec = cull_rec_at(cr, tile);  // issued ahead of the vector loads: the latencies overlap
    tile_x = (int)crec.tile_x;
    tile_y = (int)(crec.tile_y & ~kCullRecFull);
  } else if constexpr (CACHED) {
    if (tile >= ntiles) return;  // the same test as below, before the record is read
    trec = tile_rec_at(tr, tile);  // issued ahead of ray_cache_load: the two latencies overlap
    tile_x = (int)trec.tile_x;
    tile_y = (int)trec.tile_y;
  } else {
    tile_y = tile / f.tiles_x;  // f.tiles_x = ceil(sub_w / (8 R)) for this kernel
    tile_x = tile - tile_y * f.tiles_x;
    if (tile_y * kTile >= f.sub_rows) return;  // grid rounding; uniform per wave
  }
  probe.tile_begin();
  [[maybe_unused]] const int b = f.sub_row0 + tile_y * kTile + (lane >> 3);
  const int b_end = f.sub_row0 + f.sub_rows;
  [[maybe_unused]] const int bc = b < b_end ? b : b_end - 1;
  [[maybe_unused]] const int j = CACHED ? 0 : subset_index<SS>(f.ystart, f.yadd, bc);
  const float l0 = f.first_l;
  Rays<R> ray;  // iters: DUMP and AUX only, the host's first trip included
  uint64_t m_end = 0;  // the wave's culling mask, for the probe's tile_end
  [[maybe_unused]] uint32_t hit_w[(HIT == 1 || HIT == 3 || CF) ? R : 1];
  if constexpr (CF) {  // as below, with each record's moving bit kept for the compact record
    const bool moving = texel_load_w<R>(xr, tile, lane, ray.draw, ray.pz, hit_w);
    if (__builtin_amdgcn_ballot_w64(moving) != 0 && lane == 0) atomicOr(f.status, 1);
  } else if constexpr (HIT == 4) {
    // ray.draw holds the records' texel indices from here on, ray.pz the brightness
    const bool moving = texel_load<R>(xr, tile, lane, ray.draw, ray.pz);
    if (__builtin_amdgcn_ballot_w64(moving) != 0 && lane == 0) atomicOr(f.status, 1);
  } else if constexpr (HIT == 3) {
    const bool moving = hit_load_w<R>(hr, tile, lane, ray.px, ray.py, ray.pz, ray.draw, hit_w);
    if (__builtin_amdgcn_ballot_w64(moving) != 0 && lane == 0) atomicOr(f.status, 1);
  } else if constexpr (HIT == 2) {
    // every lane, clamped duplicates included: a duplicate is some stored pixel's ray again, so
    // "some ray of the wave still moved" is what march_wave's own test saw.  ray.px, py, pz hold
    // the records' fu, fw and brightness from here on (shade_texel's FRAC), not a position.
    const bool moving = hit_load<R>(hr, tile, lane, ray.px, ray.py, ray.pz, ray.draw);
    if (__builtin_amdgcn_ballot_w64(moving) != 0 && lane == 0) atomicOr(f.status, 1);
  } else {
    if constexpr (CULLED) cwin = cw[cull_win_at(tile, lane)];  // beside the directions' loads
    if constexpr (CACHED) ray_cache_load<R>(rc, tile, lane, ray.dx, ray.dy, ray.dz);
#pragma unroll
    for (int r = 0; r < R; r++) {
      if constexpr (!CACHED) {
        const int a = tile_x * R * kTile + r * kTile + (lane & 7);
        const int ac = a < f.sub_w ? a : f.sub_w - 1;
        primary_dir(f, subset_index<SS>(f.xstart, f.xadd, ac), j, ray.dx[r], ray.dy[r], ray.dz[r]);
      }
      ray.px[r] = f.cam[0] + ray.dx[r] * l0;
      ray.py[r] = f.cam[1] + ray.dy[r] * l0;
      ray.pz[r] = f.cam[2] + ray.dz[r] * l0;
      ray.draw[r] = f.first_draw;
      ray.iters[r] = 1;
      ray.mv[r] = l0 > 0.0f ? 1.0f : 0.0f;
      ray.tacc[r] = l0;  // along-ray distance marched (binary32 sum of the steps)
    }
    // The windows are first used inside the march's window path, and left alone the compiler sinks
    // their load down there; a use here keeps it above, ahead of the directions' loads, whose
    // arrival (in order) the positions above have already waited for.  R >= 3 only (the wide
    // tiles of large frames): 4K 64 spheres 122.7 -> 122.1 us with it; at R = 2 a wave with at
    // most kSlots culled spheres never reads its windows, and loading them for every wave cost
    // the 1080p 10-sphere frame 3 % (profiles/ab/r9c_ab3_window_load.txt).
    if constexpr (CULLED && R >= 3) {
      __asm__ volatile("" : : "v"(cwin.lo), "v"(cwin.hi));
      if constexpr (LIST) __asm__ volatile("" : : "v"(cwin.cidx));
    }
    const bool windowed = f.cull && l0 > 0.0f;
    bool culled = windowed;  // else every step visits every sphere
    uint64_t m = 0;          // culled spheres (LIST: culled-list entries)
    float lo = -__builtin_inff(), hi = __builtin_inff();
    int cidx = lane;         // sphere of culled-list entry `lane`
    if constexpr (CULLED) {
      // No branch on `windowed`: for a launch that does not cull, k_cull_fill stored the values
      // set above (under a branch the compiler sinks the window load into it, its whole latency
      // exposed right before the march, and copies the rays' registers at the join).
      m = (uint64_t)crec.m_lo | ((uint64_t)crec.m_hi << 32);
      lo = cwin.lo;
      hi = cwin.hi;
      if constexpr (LIST) {
        cidx = cwin.cidx;
        culled = windowed && (crec.tile_y & kCullRecFull) == 0;
      }
    } else if (windowed) {
      Cone cone;
      if constexpr (CACHED) {
        cone.ax = trec.ax; cone.ay = trec.ay; cone.az = trec.az;
        cone.sin_t = trec.sin_t; cone.cos_t = trec.cos_t;
        cone.wide = trec.wide != 0;
      } else {
        cone = tile_cone<R, SS>(f, tile_x, tile_y, lane, ray.dx, ray.dy, ray.dz);
      }
      cull_wave<LIST>(f, sph, cone, lane, culled, m, lo, hi, cidx);
    }
    ray = march_wave<R, LIST, DUMP || AUX>(f, sph, lane, probe, culled, m, lo, hi, cidx, ray);
    if constexpr (HIT == 1) {  // the record's fourth dword; the tail below stores it with its own three
#pragma unroll
      for (int r = 0; r < R; r++) hit_w[r] = hit_pack_draw(ray.draw[r], ray.mv[r] > 0.0f);
    }
    m_end = m;
  }
  const int trips = READS ? 0 : ray.trips;  // (no march; `ray` holds the loaded results only)
  if constexpr (!READS) {
    if (f.tile_cost && lane == 0) store_cost(f.tile_cost, tile, tile_bucket((uint32_t)trips), cls, f.cost_diff);
  }
  // Pixel (a, b) of ray r, recomputed here from a fresh lane id (mbcnt, so that the
  // compiler does not reuse the kernel entry's values): kept from there, the columns sat
  // in registers through the whole march, and at R = 4 one of them was spilled.
  const int lane_s = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int b_s = f.sub_row0 + tile_y * kTile + (lane_s >> 3);
  auto col = [&](int r) { return tile_x * R * kTile + r * kTile + (lane_s & 7); };
  auto valid = [&](int r) { return col(r) < f.sub_w && b_s < b_end; };
  // the row's first pixel, once per lane (inside each slot's store branch the compiler
  // recomputed the 64-bit row offset, three quarter-rate multiplies per slot)
  // (SS > 0: the output pixel of sample (a, b) is (a >> SS, (b - sub_row0) >> SS))
  uint32_t* const row_out = f.out + (long long)((b_s - f.sub_row0) >> SS) * f.out_pitch;
  // the output column's element offset in its row (PLACE: xstride apart; < 2^31, the host checks)
  auto col_out = [&](int r) {
    if constexpr (PLACE) return (col(r) >> SS) * xstride;
    else return col(r) >> SS;
  };
  auto px_out = [&](int r) { return row_out + col_out(r); };
  // AUX: each plane's row likewise (null planes: wave-uniform, never stored)
  [[maybe_unused]] float* depth_row = nullptr;
  [[maybe_unused]] int32_t* sphere_row = nullptr;
  [[maybe_unused]] int32_t* steps_row = nullptr;
  if constexpr (AUX) {
    const long long row = (long long)((b_s - f.sub_row0) >> SS);
    if (aux.depth) depth_row = aux.depth + row * aux.depth_pitch;
    if (aux.sphere) sphere_row = aux.sphere + row * aux.sphere_pitch;
    if (aux.steps) steps_row = aux.steps + row * aux.steps_pitch;
  }
  if constexpr (!P::kShade) {  // timing probe (sfrt_probe.h): the march without the shading tail
#pragma unroll
    for (int r = 0; r < R; r++)
      if (valid(r))
        probe.march_only(px_out(r), __float_as_uint(ray.px[r]) ^ __float_as_uint(ray.py[r]) ^
                                        __float_as_uint(ray.pz[r]) ^ (uint32_t)ray.draw[r]);
  } else {
    // Shading: the R records gathered first, then the R texel indices, the R texel
    // loads back to back, and the stores.  Edge lanes shade their duplicates too
    // (same values as the real pixel) and store nothing.
    [[maybe_unused]] SphereRec d[HIT == 4 ? 1 : R];
    if constexpr (HIT != 4) {
#pragma unroll
      for (int r = 0; r < R; r++)  // draw < n <= 1024: a 32-bit byte offset from the records' base
        d[r] = *(const SphereRec*)((const char*)sph + (uint32_t)ray.draw[r] * (uint32_t)sizeof(SphereRec));
    }
    Shading sh[R];
    PixelDump dl[DUMP ? R : 1];
#pragma unroll
    for (int r = 0; r < R; r++) {
      if constexpr (HIT == 4) {  // the texel record is what shade_texel left: no SphereRec is read
        sh[r].outside = texel_outside((uint32_t)ray.draw[r]);
        sh[r].tex = sh[r].outside ? 0u : (uint32_t)ray.draw[r];  // (some texel of the atlas; unused)
        sh[r].brightness = ray.pz[r];
      } else {
        sh[r] = shade_texel<P, AUX, false, HIT == 2 || HIT == 3>(f, d[HIT == 4 ? 0 : r], ray.px[r], ray.py[r], ray.pz[r], DUMP ? &dl[DUMP ? r : 0] : nullptr);
      }
    }
    // every lane, clamped duplicates included, as the reading kernels load them
    if constexpr (HIT == 1) hit_store<R>(hr, tile, lane_s, sh, hit_w);
    if constexpr (HIT == 3) texel_store<R>(xr, tile, lane_s, sh, hit_w);
    if constexpr (CF) compact_store<R>(cf, tile, lane_s, sh, hit_w, rep, classes);
    // AUX: ray r's plane values beside its colour store (plain vector stores)
    [[maybe_unused]] auto aux_store = [&](int r) {
      const int c = col_out(r);
      if (aux.depth) depth_row[c] = sh[r].depth;
      if (aux.sphere) sphere_row[c] = ray.draw[r];
      if (aux.steps) steps_row[c] = ray.iters[r];
    };
    uint32_t texel[R];
#pragma unroll
    for (int r = 0; r < R; r++) texel[r] = f.tex[sh[r].tex];
    // k_shade_texels<4, *>: all four texels before the first is used.  Left alone the compiler
    // issues three loads here and sinks the first slot's into that slot's store branch, where
    // the wave waits out a third memory trip (records, three texels, one texel); as one operand
    // list the four are issued back to back and waited for once.  4K static 16.7 -> 15.8 us,
    // 256 spheres 27.5 -> 26.6 (DESIGN.md 5 "Texel cache"); R < 4 was not tried and is left to
    // the compiler.
    if constexpr (HIT == 4 && R == 4) {
      __asm__ volatile("" : "+v"(texel[0]), "+v"(texel[1]), "+v"(texel[2]), "+v"(texel[3]));
    }
    if constexpr (SS > 0) {
      // Box filter, out_c = (sum of the S*S samples' c + S*S/2) >> log2(S*S) for each of the
      // four channels: every lane shades its sample (edge lanes their duplicates) with the
      // status bit per sample as below, then the whole wave adds across each S x S group.
      // A dword is split into two words of 16-bit fields (r, b and g, a: 16 * 255 fits), so
      // two sums serve four channels; the shift moves a field's low bits into the field
      // below, above its bit 8, where the mask drops them.
      constexpr uint32_t kLow = (1u << SS) - 1u;
      constexpr uint32_t kHalf = (1u << (2 * SS - 1)) * 0x00010001u;
      const bool leader = ((lane_s & kLow) | ((lane_s >> 3) & kLow)) == 0;
      uint32_t rgba[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (valid(r) && sh[r].outside) atomicOr(f.status, 2);
        rgba[r] = shade_rgba(sh[r].outside ? 0u : texel[r], sh[r].brightness);
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t rb = group_sum_u32<SS>(rgba[r] & 0x00ff00ffu);
        const uint32_t ga = group_sum_u32<SS>((rgba[r] >> 8) & 0x00ff00ffu);
        const uint32_t out = (((rb + kHalf) >> (2 * SS)) & 0x00ff00ffu) |
                             ((((ga + kHalf) >> (2 * SS)) & 0x00ff00ffu) << 8);
        if (leader && valid(r)) {
          *px_out(r) = out;
          if constexpr (AUX) aux_store(r);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (valid(r)) {
          if (sh[r].outside) atomicOr(f.status, 2);  // the reference would read outside the image
          const uint32_t rgba = shade_rgba(sh[r].outside ? 0u : texel[r], sh[r].brightness);
          if constexpr (!DUMP) {
            *px_out(r) = rgba;
            if constexpr (AUX) aux_store(r);
          } else {  // the listed pixel's record, if it is listed (no frame store)
            const long long pid = (long long)(b_s - f.sub_row0) * f.sub_w + col(r);
            int q = 0, qe = dmp.npix;  // first entry >= pid
            while (q < qe) {
              const int mid = (q + qe) >> 1;
              if (dmp.pix[mid] < pid) q = mid + 1;
              else qe = mid;
            }
            if (q < dmp.npix && dmp.pix[q] == pid) {
              PixelDump& o = dl[r];
              o.pos[0] = ray.px[r]; o.pos[1] = ray.py[r]; o.pos[2] = ray.pz[r];
              o.draw = ray.draw[r];
              o.iters = ray.iters[r];
              o.rgba = rgba;
              dmp.out[q] = o;
            }
          }
        }
      }
    }
  }
  probe.tile_end(px_out(0), lane_s, valid(0), trips, slot, m_end);
}

// n <= 64: the records travel in the kernel-argument segment.  8 waves/SIMD: <= 64
// VGPRs (R = 4 needs 60; measured equal to 7 waves when it spilled one, ab/r2_ab10).
template <int R>
__global__ __launch_bounds__(64, 8) void k_trace_window_r(InlineArgs args) {
  trace_tile_window_r<R, false, false, ActiveProbe>(args.f, args.s, DumpArgs{});
}

// n > 64: the records in device memory (f.spheres, read with scalar loads: rec_at), the
// culled list per wave.  61 VGPRs at R = 4 (8 waves/SIMD).
template <int R>
__global__ __launch_bounds__(64) void k_trace_window_list(FrameRec f) {
  trace_tile_window_r<R, true, false, ActiveProbe>(f, f.spheres, DumpArgs{});
}

// The supersampling instantiations of both (SFRT_OPT_SUPERSAMPLE 2 and 4: SS = 1, 2), kernels
// of their own so that the two above keep their names and their code.
template <int R, int SS>
__global__ __launch_bounds__(64, 8) void k_trace_window_r_ss(InlineArgs args) {
  trace_tile_window_r<R, false, false, ActiveProbe, SS>(args.f, args.s, DumpArgs{});
}
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_list_ss(FrameRec f) {
  trace_tile_window_r<R, true, false, ActiveProbe, SS>(f, f.spheres, DumpArgs{});
}

// The ray cache's kernels (sfrt_raycache.h), again of their own.  k_ray_fill: one wave per tile
// of the grid f.tiles_x x ceil(sub_rows / 8), row-major, stores the directions the kernels
// above compute for that tile (the same primary_dir on the same indices under the same flags:
// the same bits) and, from lane 0, the tile's record (the same tile_cone on the same inputs).
// The _rc kernels are the four above with the directions loaded from rc and the cone from tr.
template <int R, int SS>
__global__ __launch_bounds__(64) void k_ray_fill(FrameRec f, float* __restrict__ rc,
                                                 TileRec* __restrict__ tr) {
  const int lane = threadIdx.x & 63;
  const int tile = (int)blockIdx.x;
  const int tile_y = tile / f.tiles_x;
  const int tile_x = tile - tile_y * f.tiles_x;
  if (tile_y * kTile >= f.sub_rows) return;
  float dx[R], dy[R], dz[R];
  tile_dirs<R, SS>(f, tile_x, tile_y, lane, dx, dy, dz);
  ray_cache_store<R>(rc, tile, lane, dx, dy, dz);
  const Cone cone = tile_cone<R, SS>(f, tile_x, tile_y, lane, dx, dy, dz);  // every lane: wave ops
  if (lane == 0) tile_rec_store(tr, tile, tile_x, tile_y, cone);
}
template <int R, int SS>
__global__ __launch_bounds__(64, 8) void k_trace_window_r_rc(InlineArgs args,
                                                             const float* __restrict__ rc,
                                                             const TileRec* tr) {
  trace_tile_window_r<R, false, false, ActiveProbe, SS, true>(args.f, args.s, DumpArgs{}, rc, tr);
}
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_list_rc(FrameRec f,
                                                             const float* __restrict__ rc,
                                                             const TileRec* tr) {
  trace_tile_window_r<R, true, false, ActiveProbe, SS, true>(f, f.spheres, DumpArgs{}, rc, tr);
}

// The cull cache's kernels (sfrt_raycache.h CullRec, ChainCaches), of their own once more.
// k_cull_fill: one wave per tile of the same grid runs the trace kernels' own cull_wave on the
// cone of the tile's record, from the launch's own frame and sphere records under the same
// flags (the same bits), and stores what it leaves: the lane's window (and list entry), and from
// lane 0 the mask with the tile's grid position.  A launch that does not cull (f.cull off, or a
// camera inside no sphere: first_l = +0) stores the values such a launch starts from.  The
// pixels per lane and the supersampling factor reach the cull through the tile record alone, so
// the kernel is not instantiated for them.
// The _cc kernels are the _rc ones with the cull loaded as well.
template <bool LIST>
__device__ __forceinline__ void cull_fill_wave(const FrameRec& f, const SphereRec* sph,
                                               const TileRec* tr, CullRec* __restrict__ cr,
                                               CullLane<LIST>* __restrict__ cw) {
  const int lane = threadIdx.x & 63;
  const int tile = (int)blockIdx.x;  // the grid is exactly the tiles
  const TileRec trec = tile_rec_at(tr, tile);
  const bool windowed = f.cull && f.first_l > 0.0f;
  bool culled = windowed;
  uint64_t m = 0;
  float lo = -__builtin_inff(), hi = __builtin_inff();
  int cidx = lane;
  if (windowed) {
    Cone cone;
    cone.ax = trec.ax; cone.ay = trec.ay; cone.az = trec.az;
    cone.sin_t = trec.sin_t; cone.cos_t = trec.cos_t;
    cone.wide = trec.wide != 0;
    cull_wave<LIST>(f, sph, cone, lane, culled, m, lo, hi, cidx);
  }
  CullLane<LIST> win;
  win.lo = lo;
  win.hi = hi;
  if constexpr (LIST) win.cidx = cidx;
  cw[cull_win_at(tile, lane)] = win;
  if (lane == 0) {
    CullRec c;
    c.m_lo = (uint32_t)m;
    c.m_hi = (uint32_t)(m >> 32);
    c.tile_x = trec.tile_x;
    c.tile_y = trec.tile_y | ((windowed && !culled) ? kCullRecFull : 0u);
    cr[tile] = c;
  }
}
template <bool LIST>
__global__ __launch_bounds__(64) void k_cull_fill(std::conditional_t<LIST, FrameRec, InlineArgs> args,
                                                  const TileRec* tr, CullRec* __restrict__ cr,
                                                  CullLane<LIST>* __restrict__ cw) {
  if constexpr (LIST) cull_fill_wave<true>(args, args.spheres, tr, cr, cw);
  else cull_fill_wave<false>(args.f, args.s, tr, cr, cw);
}
template <int R, int SS>
__global__ __launch_bounds__(64, 8) void k_trace_window_r_cc(InlineArgs args,
                                                             const float* __restrict__ rc,
                                                             const CullRec* cr, const CullWin* cw) {
  trace_tile_window_r<R, false, false, ActiveProbe, SS, true, false, false, true>(
      args.f, args.s, DumpArgs{}, rc, nullptr, AuxArgs{}, 1, cr, cw);
}
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_list_cc(FrameRec f,
                                                             const float* __restrict__ rc,
                                                             const CullRec* cr, const CullWinList* cw) {
  trace_tile_window_r<R, true, false, ActiveProbe, SS, true, false, false, true>(
      f, f.spheres, DumpArgs{}, rc, nullptr, AuxArgs{}, 1, cr, cw);
}

// The hit cache's kernels (sfrt_raycache.h HitRec, ChainCaches).  The _hf kernels are the _cc ones that
// also store their rays' march results (HIT = 1; they run once per key, so their occupancy is
// left to the compiler); k_shade_hits[_list] shade a frame from those results (HIT = 2: no march,
// see trace_tile_window_r), the records in the arguments or, n > 64, in the device ring.
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_r_hf(InlineArgs args, const float* __restrict__ rc,
                                                          const CullRec* cr, const CullWin* cw,
                                                          HitRec* __restrict__ hr) {
  trace_tile_window_r<R, false, false, ActiveProbe, SS, true, false, false, true, 1>(
      args.f, args.s, DumpArgs{}, rc, nullptr, AuxArgs{}, 1, cr, cw, hr);
}
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_list_hf(FrameRec f, const float* __restrict__ rc,
                                                             const CullRec* cr, const CullWinList* cw,
                                                             HitRec* __restrict__ hr) {
  trace_tile_window_r<R, true, false, ActiveProbe, SS, true, false, false, true, 1>(
      f, f.spheres, DumpArgs{}, rc, nullptr, AuxArgs{}, 1, cr, cw, hr);
}
template <int R, int SS>
__global__ __launch_bounds__(64, 8) void k_shade_hits(InlineArgs args, const CullRec* cr,
                                                      const HitRec* __restrict__ hr) {
  trace_tile_window_r<R, false, false, NoProbe, SS, true, false, false, true, 2>(
      args.f, args.s, DumpArgs{}, nullptr, nullptr, AuxArgs{}, 1, cr, nullptr, const_cast<HitRec*>(hr));
}
template <int R, int SS>
__global__ __launch_bounds__(64, 8) void k_shade_hits_list(FrameRec f, const CullRec* cr,
                                                           const HitRec* __restrict__ hr) {
  trace_tile_window_r<R, true, false, NoProbe, SS, true, false, false, true, 2>(
      f, f.spheres, DumpArgs{}, nullptr, nullptr, AuxArgs{}, 1, cr, nullptr, const_cast<HitRec*>(hr));
}

// The texel cache's kernels (sfrt_raycache.h TexelRec, ChainCaches).  The _tf kernels are
// k_shade_hits[_list] that also store each lane's texel record after shade_texel (HIT = 3; once per
// TexKey, so their occupancy is left to the compiler); k_shade_texels shades a frame from those
// records (HIT = 4): per ray one 8-byte load, the texel, shade_rgba, the store.  It reads no
// SphereRec, so it takes the frame record alone whatever n is and has no _list twin.
template <int R, int SS>
__global__ __launch_bounds__(64) void k_shade_hits_tf(InlineArgs args, const CullRec* cr,
                                                      const HitRec* __restrict__ hr,
                                                      TexelRec* __restrict__ xr) {
  trace_tile_window_r<R, false, false, NoProbe, SS, true, false, false, true, 3>(
      args.f, args.s, DumpArgs{}, nullptr, nullptr, AuxArgs{}, 1, cr, nullptr, const_cast<HitRec*>(hr), xr);
}
template <int R, int SS>
__global__ __launch_bounds__(64) void k_shade_hits_list_tf(FrameRec f, const CullRec* cr,
                                                           const HitRec* __restrict__ hr,
                                                           TexelRec* __restrict__ xr) {
  trace_tile_window_r<R, true, false, NoProbe, SS, true, false, false, true, 3>(
      f, f.spheres, DumpArgs{}, nullptr, nullptr, AuxArgs{}, 1, cr, nullptr, const_cast<HitRec*>(hr), xr);
}
template <int R, int SS>
__global__ __launch_bounds__(64, 8) void k_shade_texels(FrameRec f, const CullRec* cr,
                                                        const TexelRec* __restrict__ xr) {
  trace_tile_window_r<R, false, false, NoProbe, SS, true, false, false, true, 4>(
      f, nullptr, DumpArgs{}, nullptr, nullptr, AuxArgs{}, 1, cr, nullptr, nullptr, const_cast<TexelRec*>(xr));
}

// The compact layer's kernels (sfrt_raycache.h CompactRec, ChainCaches; DESIGN.md 5 "Compact
// layer").  k_shade_texels_cf is k_shade_texels<R, 0> that also stores each ray's compact record
// (compact_store; once per TexKey, its occupancy left to the compiler).
template <int R>
__global__ __launch_bounds__(64) void k_shade_texels_cf(FrameRec f, const CullRec* cr,
                                                        const TexelRec* __restrict__ xr,
                                                        CompactRec* __restrict__ cf,
                                                        const uint32_t* __restrict__ rep, uint32_t classes) {
  trace_tile_window_r<R, false, false, NoProbe, 0, true, false, false, true, 4, true>(
      f, nullptr, DumpArgs{}, nullptr, nullptr, AuxArgs{}, 1, cr, nullptr, nullptr, const_cast<TexelRec*>(xr),
      cf, rep, classes);
}

// R dwords of one lane as one access of dword alignment (a frame's base and pitch promise no
// more).  A vector, not a struct: a struct's members become R scalar stores that the compiler may
// sink and merge apart again (at R = 4 three dwords and one, the last shared with the edge path).
template <int R>
struct Dwords {
  typedef uint32_t type __attribute__((ext_vector_type(R), aligned(4)));
};

// k_shade_compact shades a frame from the compact records.  It marches nothing, so it keeps nothing
// of the marching kernels' lane map: a lane owns the R consecutive pixels row lane >> 3, columns
// tile_x * 8R + (lane & 7) * R + r.  Its R records are one load (1 KiB contiguous per wave at
// R = 4), its R pixels one store: at R = 4 a wave writes eight whole 128-byte pieces of eight rows
// with one instruction, where the marching map needs four that each write eight 32-byte pieces.
// Between them the R texel gathers and the R gathers of the classes' brightnesses (rep[class],
// BrightClasses::rep) and shade_rgba.
// A tile that crosses the right edge stores per pixel under `valid`; its edge lanes load the
// duplicates k_shade_texels_cf stored for them and store nothing.  Status bit 0 comes from the
// moving bits, bit 2 from the sentinel of a valid lane.
// The frame record is the only argument.  A reading launch takes no part in the tile order, and
// launch_trace puts what this kernel reads where that and the records would be: f.tile_order the
// compact records, f.prev_cost the cull records, f.spheres the class table.
template <int R>
__global__ __launch_bounds__(64, 8) void k_shade_compact(FrameRec f) {
  const int tile = (int)blockIdx.x;
  const int tiles_y = (f.sub_rows + kTile - 1) / kTile;
  if (tile >= f.tiles_x * tiles_y) return;  // (the grid is exactly the tiles)
  const CullRec crec = cull_rec_at((const CullRec*)f.prev_cost, tile);
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  using Vec = typename Dwords<R>::type;
  const Vec recv = *(const Vec*)(f.tile_order + compact_rec_at(tile, R, lane, 0));
  uint32_t rec[R];
#pragma unroll
  for (int r = 0; r < R; r++) rec[r] = recv[r];
  const float* __restrict__ rep = (const float*)f.spheres;
  const int tile_x = (int)crec.tile_x;
  const int tile_y = (int)(crec.tile_y & ~kCullRecFull);
  const int row = tile_y * kTile + (lane >> 3);  // of the band
  const int col0 = tile_x * R * kTile + (lane & 7) * R;
  bool moving = false, outside[R];
  uint32_t texel[R];
  float bright[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    moving = moving || compact_moving(rec[r]);
    outside[r] = compact_outside(rec[r]);
    texel[r] = f.tex[outside[r] ? 0u : compact_tex(rec[r])];  // (some texel of the atlas; unused)
    bright[r] = rep[compact_class(rec[r])];
  }
  // (the gathers are left to the compiler: one operand list that forces all 2R before the first
  // use, k_shade_texels<4, 0>'s remedy, measured slower here -- DESIGN.md 5 "Compact layer")
  if (__builtin_amdgcn_ballot_w64(moving) != 0 && lane == 0) atomicOr(f.status, 1);
  if (row >= f.sub_rows) return;
  uint32_t* const px = f.out + (long long)row * f.out_pitch + col0;
  uint32_t rgba[R];
  bool bad = false;
#pragma unroll
  for (int r = 0; r < R; r++) {
    bad = bad | (outside[r] & (col0 + r < f.sub_w));
    rgba[r] = shade_rgba(outside[r] ? 0u : texel[r], bright[r]);
  }
  if (bad) atomicOr(f.status, 2);  // the reference would read outside the image
  if (col0 + R <= f.sub_w) {
    Vec v;
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = rgba[r];
    *(Vec*)px = v;
  } else {
#pragma unroll
    for (int r = 0; r < R; r++)
      if (col0 + r < f.sub_w) px[r] = rgba[r];
  }
}

// The pixel layer's one kernel (sfrt_raycache.h PixelKey, ChainCaches; DESIGN.md 5 "Pixel
// layer"): a band of finished pixels between the caller's frame (base and pitch the launch's) and
// the layer (rows packed), TO_FRAME from the layer, else into it.  No march, no tiles, no CullRec:
// the geometry is the arguments'.  A row is `chunks` whole 16-byte chunks (Dwords<4>: dword
// alignment, whatever the base, the pitch and the width) and, where width % 4 != 0, one tail unit
// that goes per pixel; unit g of the launch is unit g % units_per_row of row g / units_per_row.  A
// lane takes CH units WG apart, so that a wave's CH accesses are contiguous each, and issues all
// their loads before its first store.  NT: the layer is loaded non-temporally (TO_FRAME only).
// The launch's first lane ORs the layer's status word into the world's when it is not zero.
struct PixelCopyArgs {
  uint32_t* frame;     // the band's first pixel
  uint32_t* layer;     // width * rows pixels
  long long pitch;     // of the frame, in pixels
  int* layer_status;
  int* world_status;
  uint32_t width, rows;
  uint32_t chunks;     // width / 4
  uint32_t units_per_row;  // chunks + (width % 4 != 0)
  uint32_t units;      // rows * units_per_row (< 2^31: launch_trace)
  uint32_t pad;        // 64 bytes, one cache line: the scalar loads are issued together, one wait
};
static_assert(sizeof(PixelCopyArgs) == 64, "one line of kernel arguments");

template <bool TO_FRAME, int WG, int CH, bool NT>
__global__ __launch_bounds__(WG) void k_pixels_copy(PixelCopyArgs a) {
  using Vec = typename Dwords<4>::type;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) {
    const int st = *a.layer_status;
    if (st != 0) atomicOr(a.world_status, st);
  }
  const uint32_t g0 = blockIdx.x * (uint32_t)(WG * CH) + tid;
  const uint32_t tail = a.width - a.chunks * 4u;
  const uint32_t* src[CH];
  uint32_t* dst[CH];
  uint32_t count[CH];  // 4: a whole chunk; 1..3: the row's tail; 0: past the band
  Vec whole[CH];
  uint32_t part[CH][3];
#pragma unroll
  for (int k = 0; k < CH; k++) {
    const uint32_t g = g0 + (uint32_t)(k * WG);
    const uint32_t row = g / a.units_per_row, unit = g - row * a.units_per_row;
    uint32_t* const fr = a.frame + (long long)row * a.pitch + unit * 4u;
    uint32_t* const la = a.layer + (size_t)row * a.width + unit * 4u;
    src[k] = TO_FRAME ? la : fr;
    dst[k] = TO_FRAME ? fr : la;
    count[k] = g >= a.units ? 0u : unit < a.chunks ? 4u : tail;
  }
#pragma unroll
  for (int k = 0; k < CH; k++) {
    if (count[k] == 4u) {
      if constexpr (NT && TO_FRAME) whole[k] = __builtin_nontemporal_load((const Vec*)src[k]);
      else whole[k] = *(const Vec*)src[k];
    } else {
#pragma unroll
      for (uint32_t p = 0; p < 3; p++)
        if (p < count[k]) part[k][p] = src[k][p];
    }
  }
#pragma unroll
  for (int k = 0; k < CH; k++) {
    if (count[k] == 4u) {
      *(Vec*)dst[k] = whole[k];
    } else {
#pragma unroll
      for (uint32_t p = 0; p < 3; p++)
        if (p < count[k]) dst[k][p] = part[k][p];
    }
  }
}

// The DUMP instantiations of both (sfrt_world_trace_points): the shipped march and
// shading, with the float intermediates of listed pixels written out (never probed).
template <int R>
__global__ __launch_bounds__(64) void k_trace_window_r_dump(InlineArgs args, DumpArgs d) {
  trace_tile_window_r<R, false, true, NoProbe>(args.f, args.s, d);
}
template <int R>
__global__ __launch_bounds__(64) void k_trace_window_list_dump(FrameRec f, DumpArgs d) {
  trace_tile_window_r<R, true, true, NoProbe>(f, f.spheres, d);
}

// The AUX instantiations of both, at every factor (sfrt_world_render_band_aux; never probed).
// Four step counters more than the plain kernels carry: no occupancy bound.
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_r_aux(InlineArgs args, AuxArgs a) {
  trace_tile_window_r<R, false, false, NoProbe, SS, false, true>(args.f, args.s, DumpArgs{}, nullptr,
                                                                 nullptr, a);
}
template <int R, int SS>
__global__ __launch_bounds__(64) void k_trace_window_list_aux(FrameRec f, AuxArgs a) {
  trace_tile_window_r<R, true, false, NoProbe, SS, false, true>(f, f.spheres, DumpArgs{}, nullptr,
                                                                nullptr, a);
}

// The placing instantiations (sfrt_world_render_subset[_aux]; never probed): one
// family, AUX its flag, the planes and the column stride in arguments of their own.  The plain
// ones keep k_trace_window_r's bound while they fit it; the plane-writing ones carry the AUX
// kernels' step counters and, like them, take no occupancy bound.
template <int R, int SS, bool AUX>
__global__ __launch_bounds__(64, AUX ? 1 : 8) void k_trace_place_r(InlineArgs args, AuxArgs a, int xstride) {
  trace_tile_window_r<R, false, false, NoProbe, SS, false, AUX, true>(args.f, args.s, DumpArgs{}, nullptr,
                                                                      nullptr, a, xstride);
}
template <int R, int SS, bool AUX>
__global__ __launch_bounds__(64) void k_trace_place_list(FrameRec f, AuxArgs a, int xstride) {
  trace_tile_window_r<R, true, false, NoProbe, SS, false, AUX, true>(f, f.spheres, DumpArgs{}, nullptr,
                                                                     nullptr, a, xstride);
}

// The view batches (sfrt_world_render_views[_aux]; never probed): workgroup (x, y)
// is tile x of view y.  The view's record is read from the device table once, at entry, like a
// sphere record (rec_at): the table is written only by the staging copy that precedes the launch
// on its stream, the address is wave-uniform, so through the constant address space the fields
// the body uses arrive by scalar loads, as the band kernels' arrive from their arguments.  The
// body then runs on that copy as it runs on a band's arguments: row-major (the order fields are
// constants here, so the sorter, the order lookup and the class store fold away), directions
// computed, nothing dumped.  n <= 64 takes the non-list body -- the list body's lookahead needs
// sphere 63 -- with the records in the table, where 64 are readable, in place of the arguments.
__device__ __forceinline__ ViewRec view_rec_at(const ViewRec* p, uint32_t view) {
  const __attribute__((address_space(4))) uint32_t* q =
      (const __attribute__((address_space(4))) uint32_t*)(
          (const __attribute__((address_space(4))) char*)p + (size_t)view * sizeof(ViewRec));
  uint32_t w[sizeof(ViewRec) / 4];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(ViewRec) / 4); i++) w[i] = q[i];
  ViewRec r;
  __builtin_memcpy(&r, w, sizeof r);
  return r;
}
// The plain n <= 64 ones keep k_trace_window_r's bound; the others take none, as the kernels
// they mirror.
template <int R, int SS, bool LIST, bool AUX>
__global__ __launch_bounds__(64, (LIST || AUX) ? 1 : 8) void k_trace_views(const ViewRec* views) {
  ViewRec v = view_rec_at(views, blockIdx.y);
  v.f.tile_order = nullptr;
  v.f.tile_cost = nullptr;
  v.f.prev_cost = nullptr;
  v.f.next_order = nullptr;
  trace_tile_window_r<R, LIST, false, NoProbe, SS, false, AUX>(v.f, v.f.spheres, DumpArgs{}, nullptr,
                                                              nullptr, AUX ? v.a : AuxArgs{});
}

// ---- Ray batches: SphereWorld::Raycast for caller-supplied rays (sfrt_world_cast_rays;
// DESIGN.md 18) ----
//
// Unit direction of a caller's ray (VNormalize, SphereWorld.cpp:330-333, :340-343):
// (x, y, z) / sqrtf(s) with s = (x*x + y*y) + z*z a finite normal number, the correctly rounded
// root and three correctly rounded divisions.  Unlike primary_dir's, the operands are
// anything a caller passes: div_inrange only when every lane's components and length lie in
// [2^-40, 2^40), the compiler's `/` in a kept branch otherwise.
__device__ __forceinline__ void ray_dir(float x, float y, float z, float s, float& dx, float& dy,
                                        float& dz) {
  const float len = sqrt_cr(s);
  if ((ballot_bad_operand(x) | ballot_bad_operand(y) | ballot_bad_operand(z) |
       ballot_bad_operand(len)) == 0) {
    const float sd = div_seed(len);
    dx = div_inrange(x, len, sd);
    dy = div_inrange(y, len, sd);
    dz = div_inrange(z, len, sd);
  } else {
    const float l = keep_branch(len);
    dx = x / l;
    dy = y / l;
    dz = z / l;
  }
}

// Cone of a wave's 64 unit directions, all from one apex: the axis is lane 27's direction (the
// middle of an 8x8-tile-major batch; any lane's serves), the half-angle's sine the wave's
// largest |d x a| plus tile_cone_r's slack (d and a are unit to a few 1e-8, far inside it), and
// the wave is wide when some lane is more than 60 degrees off the axis.  Every ray of the wave
// lies in this cone by construction, which is all cull_window's argument needs of it.
__device__ __forceinline__ Cone dirs_cone(float dx, float dy, float dz) {
  const float ax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dx), 27));
  const float ay = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dy), 27));
  const float az = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dz), 27));
  const float cx = dy * az - dz * ay, cy = dz * ax - dx * az, cz = dx * ay - dy * ax;
  const float sin_l = sqrt_cull((cx * cx + cy * cy) + cz * cz);
  Cone c;
  c.ax = ax; c.ay = ay; c.az = az;
  c.sin_t = fminf(1.0f, __uint_as_float(wave_max_u32(__float_as_uint(sin_l))) + 1e-5f);
  c.cos_t = sqrt_cull(fmaxf(0.0f, 1.0f - c.sin_t * c.sin_t));
  c.wide = __builtin_amdgcn_ballot_w64(!(((dx * ax + dy * ay) + dz * az) >= 0.5f)) != 0;
  return c;
}

// One wave per 64 consecutive rays of the batch, ray q = 64 * block + lane; the lanes past the
// batch's end trace a duplicate of its last ray and store nothing.  The cull and the march are
// the frame kernels' at one ray per lane (cull_wave, march_wave), with what the frame gives a
// tile replaced by what the batch gives a wave:
//  * the direction is loaded and normalised (ray_dir), not derived from a pixel;
//  * OWN (origins given): every ray starts at its own origin, so the host's first iteration
//    (first_l, first_draw: the trip from cam) does not apply -- the first trip runs here, steps
//    count from 0 -- and neither does the drift bound behind cull_margin: every step visits
//    every sphere in index order;
//  * shared origin: the rays start at f.cam as a frame's do, and a wave culls against the cone
//    of its own directions (dirs_cone), coherent or not (a scattered wave is wide: cull_window
//    then keeps every sphere that can pass at all, with an unbounded window);
//  * an invalid ray (a non-finite component, or s not a finite normal number) holds still at a
//    NaN position, where no sphere passes (NaN < s_pass is false), so every step moves it by +0
//    and counts nothing; its outputs are the invalid ray's constants.  A wave with such a lane
//    does not cull (its cone would have to leave the lane out).
// SHADE: rgba is requested -- the shading tail with the ray's origin in cam's place; without
// it depth is the one root.  Each output is stored under a wave-uniform null test.
template <bool LIST, bool SHADE, bool OWN>
__device__ __forceinline__ void cast_rays_wave(const FrameRec& f, const SphereRec* __restrict__ sph,
                                               const RayArgs& a) {
  constexpr int R = 1;
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * 64 + lane;
  const long long qc = q < a.count ? q : a.count - 1;
  const float* __restrict__ dp = a.dirs + 3 * qc;
  const float rx = dp[0], ry = dp[1], rz = dp[2];
  float ox = f.cam[0], oy = f.cam[1], oz = f.cam[2];
  if constexpr (OWN) {
    const float* __restrict__ op = a.origins + 3 * qc;
    ox = op[0]; oy = op[1]; oz = op[2];
  }
  const float s = (rx * rx + ry * ry) + rz * rz;  // finite only if every component is
  const bool ok = s >= 0x1.0p-126f && s < __builtin_inff() &&
                  __builtin_fabsf(ox) < __builtin_inff() && __builtin_fabsf(oy) < __builtin_inff() &&
                  __builtin_fabsf(oz) < __builtin_inff();
  const bool any_invalid = __builtin_amdgcn_ballot_w64(!ok) != 0;
  const float l0 = OWN ? 0.0f : f.first_l;
  Rays<R> ray;
  // an invalid lane normalises (1, 0, 0): its operands keep the wave on ray_dir's short path
  ray_dir(ok ? rx : 1.0f, ok ? ry : 0.0f, ok ? rz : 0.0f, ok ? s : 1.0f, ray.dx[0], ray.dy[0], ray.dz[0]);
  if (ok) {
    // r->pos = cam.pos (:357); shared origin: plus the host's first trip (:371)
    ray.px[0] = OWN ? ox : ox + ray.dx[0] * l0;
    ray.py[0] = OWN ? oy : oy + ray.dy[0] * l0;
    ray.pz[0] = OWN ? oz : oz + ray.dz[0] * l0;
    ray.mv[0] = OWN ? 1.0f : (l0 > 0.0f ? 1.0f : 0.0f);
  } else {
    ray.dx[0] = ray.dy[0] = ray.dz[0] = 0.0f;
    ray.px[0] = ray.py[0] = ray.pz[0] = __builtin_nanf("");
    ray.mv[0] = 0.0f;
  }
  ray.draw[0] = OWN ? 0 : f.first_draw;
  ray.iters[0] = OWN ? 0 : 1;
  ray.tacc[0] = l0;
  const bool windowed = !OWN && f.cull && l0 > 0.0f && !any_invalid;
  bool culled = windowed;  // else every step visits every sphere
  uint64_t m = 0;          // culled spheres (LIST: culled-list entries)
  float lo = -__builtin_inff(), hi = __builtin_inff();
  int cidx = lane;         // sphere of culled-list entry `lane`
  if (windowed) {
    cull_wave<LIST>(f, sph, dirs_cone(ray.dx[0], ray.dy[0], ray.dz[0]), lane, culled, m, lo, hi, cidx);
  }
  NoProbe probe;
  ray = march_wave<R, LIST, true>(f, sph, lane, probe, culled, m, lo, hi, cidx, ray);
  const bool live = q < a.count;
  uint32_t rgba = 0u;
  float depth = 0.0f;
  if constexpr (SHADE) {
    // draw < n <= 1024: a 32-bit byte offset from the records' base
    const SphereRec d = *(const SphereRec*)((const char*)sph + (uint32_t)ray.draw[0] * (uint32_t)sizeof(SphereRec));
    const Shading sh = shade_texel<NoProbe, true, true>(f, d, ray.px[0], ray.py[0], ray.pz[0], nullptr, ox, oy, oz);
    const uint32_t texel = f.tex[sh.tex];
    if (live && ok && sh.outside) atomicOr(f.status, 2);  // the reference would read outside the image
    rgba = shade_rgba(sh.outside ? 0u : texel, sh.brightness);
    depth = sh.depth;
  } else if (a.depth) {  // VLength(r->pos - origin) of :375 alone
    const float bx = ray.px[0] - ox, by = ray.py[0] - oy, bz = ray.pz[0] - oz;
    depth = sqrt_cr((bx * bx + by * by) + bz * bz);
  }
  if (live) {  // an invalid ray: sphere -1, all-zero bytes elsewhere
    if (a.pos) {
      float* const o = a.pos + 3 * q;
      o[0] = ok ? ray.px[0] : 0.0f;
      o[1] = ok ? ray.py[0] : 0.0f;
      o[2] = ok ? ray.pz[0] : 0.0f;
    }
    if (a.depth) a.depth[q] = ok ? depth : 0.0f;
    if (a.sphere) a.sphere[q] = ok ? ray.draw[0] : -1;
    if (a.steps) a.steps[q] = ok ? ray.iters[0] : 0;
    if constexpr (SHADE) a.rgba[q] = ok ? rgba : 0u;
  }
}

// LIST: n > 64, the records in device memory (f.spheres) and the culled list per wave; else
// they travel in the kernel arguments, as for the frame kernels.
template <bool LIST, bool SHADE, bool OWN>
__global__ __launch_bounds__(64) void k_cast_rays(std::conditional_t<LIST, FrameRec, InlineArgs> args,
                                                  RayArgs rays) {
  if constexpr (LIST) cast_rays_wave<true, SHADE, OWN>(args, args.spheres, rays);
  else cast_rays_wave<false, SHADE, OWN>(args.f, args.s, rays);
}

}  // namespace

// Pixels per lane R of an ordered launch (adaptive tile order): the widest
// tile -- four pixels per lane (32x8), else three (24x8) -- whose grid still
// has >= 30000 tiles, about four waves per wave slot of the chip, enough for
// longest-first to balance; else two (16x8).  Measured: 4K 64 spheres 177
// (16x8) -> 173.5 (24x8) -> 172.9 us (32x8), 8K 645.6 -> 636.7 us (24x8 ->
// 32x8); 1080p 10 spheres 37.3 us at 16x8 against 39.4 / 41.0 wider.
static int ordered_rays(const FrameRec& f) {
  const long long rows = (f.sub_rows + kTile - 1) / kTile;
  const long long t4 = (long long)((f.sub_w + 4 * kTile - 1) / (4 * kTile)) * rows;
  const long long t3 = (long long)((f.sub_w + 3 * kTile - 1) / (3 * kTile)) * rows;
  return t4 >= 30000 ? 4 : t3 >= 30000 ? 3 : 2;
}

// The one kernel table, shared by launch_trace and trace_tile_key: pixels per
// lane R (k_trace_window_r for n <= 64, k_trace_window_list above).  Row-major launches
// use 16x8 tiles above kPairMinSpheres spheres and 8x8 tiles otherwise (their
// tighter cones win there); ordered launches ordered_rays for any scene (1080p,
// 10 spheres: 16x8 37.4 us against 42.0 with 8x8, which win only in row-major
// order: 45.7 vs 48.5).  f.rays (SFRT_OPT_RAYS_PER_LANE) overrides the choice.
static int trace_rays(const FrameRec& f, bool ordered) {
  if (f.rays >= 1 && f.rays <= 4) return f.rays;
  if (ordered) return ordered_rays(f);
  return f.n > kPairMinSpheres ? 2 : 1;
}

const char* trace_build_flavour() {
  return kDiagnosticBuild ? "diagnostic" : kSlots != 2 ? "ab" : SFRT_BUILD_FLAVOUR;
}

long long trace_tile_key(const FrameRec& f, long long* tiles) {
  *tiles = 0;
  const int rays = trace_rays(f, true);
  const long long tiles_x = (f.sub_w + rays * kTile - 1) / (rays * kTile);
  const long long tiles_y = (f.sub_rows + kTile - 1) / kTile;
  if (tiles_x <= 0 || tiles_y <= 0) return 0;
  *tiles = tiles_x * tiles_y;
  return (1ll << 62) | ((long long)(f.ss & 3) << 59) | ((long long)rays << 56) | (tiles_x << 28) |
         tiles_y;
}

long long trace_blocks(const FrameRec& f) {
  const long long tiles_y = (f.sub_rows + kTile - 1) / kTile;
  if (tiles_y <= 0 || f.sub_w <= 0) return 0;
  const int rays = std::min(trace_rays(f, false), trace_rays(f, true));  // the narrower tile
  const long long tiles_x = (f.sub_w + rays * kTile - 1) / (rays * kTile);
  return tiles_x * tiles_y + 1;  // + the tile-order sorter
}

namespace {

// Pixels per lane R = 1..4 and supersampling SS = 0..2 as compile-time constants: fn gets a
// std::integral_constant<int, N>.
template <class F>
void with_rays(int rays, F fn) {
  switch (rays) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    default: fn(std::integral_constant<int, 4>{}); break;
  }
}
template <class F>
void with_ss(int ss, F fn) {
  switch (ss) {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case 1: fn(std::integral_constant<int, 1>{}); break;
    default: fn(std::integral_constant<int, 2>{}); break;
  }
}

}  // namespace

namespace {

// The shipped variant of k_pixels_copy (DESIGN.md 5 "Pixel layer": the A/B of the workgroup size,
// the units per lane and the layer's load policy -- one wave per workgroup and four units per lane
// was the fastest of the six plain variants at 4K, every non-temporal one 1.6 to 3.3 us slower).
constexpr int kPixelCopyWg = 64, kPixelCopyUnits = 4;
constexpr bool kPixelCopyNt = false;

template <bool TO_FRAME, int WG, int CH, bool NT>
void launch_pixels_copy_as(const PixelCopyArgs& a, hipStream_t s, hipEvent_t ev) {
  const dim3 gr((a.units + (uint32_t)(WG * CH) - 1u) / (uint32_t)(WG * CH)), b(WG);
  if (ev) hipExtLaunchKernelGGL((k_pixels_copy<TO_FRAME, WG, CH, NT>), gr, b, 0, s, nullptr, ev, 0, a);
  else hipLaunchKernelGGL((k_pixels_copy<TO_FRAME, WG, CH, NT>), gr, b, 0, s, a);
}

// The band of f between the caller's frame and `layer` (pixel_cache_bytes of the band's output
// pixels); ev (may be null): the launch's stop event.
template <bool TO_FRAME>
int launch_pixels_copy(const FrameRec& f, uint32_t* layer, int* layer_status, hipStream_t s, hipEvent_t ev) {
  if (!pixel_copy_fits(f) || !layer || !layer_status || !f.out || !f.status) return -1;
  PixelCopyArgs a{};
  a.frame = f.out;
  a.layer = layer;
  a.pitch = f.out_pitch;
  a.layer_status = layer_status;
  a.world_status = f.status;
  a.width = (uint32_t)(f.sub_w >> f.ss);
  a.rows = (uint32_t)(f.sub_rows >> f.ss);
  a.chunks = a.width / 4u;
  a.units_per_row = a.chunks + (a.width % 4u != 0u ? 1u : 0u);
  a.units = a.rows * a.units_per_row;
#ifdef SFRT_PIXEL_AB  // an A/B build: SFRT_AB_KNOB = 100 * WG + 10 * units per lane + NT
  static const int knob = std::getenv("SFRT_AB_KNOB") ? std::atoi(std::getenv("SFRT_AB_KNOB")) : 0;
  switch (TO_FRAME ? knob : 0) {
#define SFRT_PIXEL_VARIANT(WG, CH, NT) \
    case 100 * WG + 10 * CH + NT: launch_pixels_copy_as<TO_FRAME, WG, CH, NT != 0>(a, s, ev); break;
    SFRT_PIXEL_VARIANT(64, 1, 0) SFRT_PIXEL_VARIANT(64, 2, 0)
    SFRT_PIXEL_VARIANT(256, 1, 0) SFRT_PIXEL_VARIANT(256, 2, 0) SFRT_PIXEL_VARIANT(256, 4, 0)
    SFRT_PIXEL_VARIANT(64, 1, 1) SFRT_PIXEL_VARIANT(64, 2, 1) SFRT_PIXEL_VARIANT(64, 4, 1)
    SFRT_PIXEL_VARIANT(256, 1, 1) SFRT_PIXEL_VARIANT(256, 2, 1) SFRT_PIXEL_VARIANT(256, 4, 1)
#undef SFRT_PIXEL_VARIANT
    default: launch_pixels_copy_as<TO_FRAME, kPixelCopyWg, kPixelCopyUnits, kPixelCopyNt>(a, s, ev); break;
  }
#else
  launch_pixels_copy_as<TO_FRAME, kPixelCopyWg, kPixelCopyUnits, kPixelCopyNt>(a, s, ev);
#endif
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

bool pixel_copy_fits(const FrameRec& f) {
  if (f.ss < 0 || f.ss > 2 || f.sub_w <= 0 || f.sub_rows <= 0) return false;
  const long long w = f.sub_w >> f.ss, rows = f.sub_rows >> f.ss;
  return w > 0 && rows > 0 && rows * ((w + 3) / 4) <= 0x7fffffffLL - 1024;
}

int launch_ray_fill(const FrameRec& f, float* ray_cache, TileRec* tile_recs, void* stream) {
  long long tiles = 0;
  if (!ray_cache || !tile_recs || f.ss < 0 || f.ss > 2 || trace_tile_key(f, &tiles) == 0 || tiles > 0x7fffffffLL)
    return -1;
  const int rays = trace_rays(f, true);
  FrameRec g = f;
  g.tiles_x = (f.sub_w + rays * kTile - 1) / (rays * kTile);
  const dim3 gr((unsigned)tiles), b(64);
  hipStream_t s = (hipStream_t)stream;
  with_rays(rays, [&](auto r) {
    with_ss(f.ss, [&](auto ss) {
      hipLaunchKernelGGL((k_ray_fill<decltype(r)::value, decltype(ss)::value>), gr, b, 0, s, g, ray_cache,
                         tile_recs);
    });
  });
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_cull_fill(const FrameRec& f, const SphereRec* host_spheres, const TileRec* tile_recs,
                     CullRec* cull_recs, void* cull_wins, void* stream) {
  long long tiles = 0;
  if (!tile_recs || !cull_recs || !cull_wins || f.n <= 0 || trace_tile_key(f, &tiles) == 0 ||
      tiles > 0x7fffffffLL)
    return -1;
  const bool list = f.n > kInlineSpheres;  // as launch_trace
  if (list ? !f.spheres : !host_spheres) return -1;
  const dim3 gr((unsigned)tiles), b(64);
  hipStream_t s = (hipStream_t)stream;
  if (list) {
    hipLaunchKernelGGL(k_cull_fill<true>, gr, b, 0, s, f, tile_recs, cull_recs, (CullWinList*)cull_wins);
  } else {
    InlineArgs args;
    args.f = f;
    for (int k = 0; k < f.n; k++) args.s[k] = host_spheres[k];
    hipLaunchKernelGGL(k_cull_fill<false>, gr, b, 0, s, args, tile_recs, cull_recs, (CullWin*)cull_wins);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_trace(const FrameRec& f, const SphereRec* host_spheres, void* stream,
                 const DumpArgs* dump, void* done_event, const TraceCaches* caches,
                 const AuxArgs* aux, int place_xstride) {
  const long long tiles_y = (f.sub_rows + kTile - 1) / kTile;
  if (tiles_y <= 0 || f.sub_w <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const TraceCaches c = caches ? *caches : TraceCaches{};
  const float* const ray_cache = c.dirs;
  const TileRec* const tile_recs = c.tile_recs;
  const CullRec* const cull_recs = c.cull_recs;
  const void* const cull_wins = c.cull_wins;
  HitRec* const hit_recs = c.hit_recs;
  TexelRec* const texel_recs = c.texel_recs;
  const int hit_mode = c.hit == RayAction::kRead ? 2 : c.hit == RayAction::kFill ? 1 : 0;
  // the texel cache rides on a launch that reads the hit cache: 1 also stores it, 2 shades from it
  const int texel_mode = c.texel == RayAction::kRead ? 2 : c.texel == RayAction::kFill ? 1 : 0;
  // the hit cache rides on the cull cache: 1 fills it from the marching launch, 2 shades from it
  if (hit_mode < 0 || hit_mode > 2 || (hit_mode != 0) != (hit_recs != nullptr)) return -1;
  if ((texel_mode != 0) != (texel_recs != nullptr) || (texel_mode && hit_mode != 2)) return -1;
  if (hit_mode && (!cull_recs || dump || aux || place_xstride || kDiagnosticBuild)) return -1;
  // the compact layer rides on a launch that reads the texel records: 1 also stores it
  // (k_shade_texels_cf), 2 shades from it (k_shade_compact); never supersampled
  const int compact_mode = c.compact == RayAction::kRead ? 2 : c.compact == RayAction::kFill ? 1 : 0;
  if ((compact_mode != 0) != (c.compact_recs != nullptr)) return -1;
  if (compact_mode && (texel_mode != 2 || f.ss != 0 || !c.bright_rep || c.bright_classes == 0 ||
                       c.bright_classes >= kCompactClassLimit))
    return -1;
  // the pixel layer rides on a launch that reads the texel records (and the compact ones, if it has
  // them): 1 that launch with the layer's status word, then its band copied into the layer; 2 the
  // band copied out of it and nothing else
  const int pixel_mode = c.pixel == RayAction::kRead ? 2 : c.pixel == RayAction::kFill ? 1 : 0;
  if ((pixel_mode != 0) != (c.pixels != nullptr)) return -1;
  if (pixel_mode && (texel_mode != 2 || compact_mode == 1 || !c.pixel_status || !pixel_copy_fits(f))) return -1;
  if (pixel_mode == 2)
    return launch_pixels_copy<true>(f, c.pixels, c.pixel_status, s,
                                    f.n > kInlineSpheres ? (hipEvent_t)done_event : nullptr);
  // (2: the caller linked nothing of the tile order into f, but the grid is the ordered one)
  const bool ordered = hit_mode == 2 || f.tile_cost != nullptr;  // linked into the tile-order chain
  const int rays = trace_rays(f, ordered);
  FrameRec g = f;
  g.tiles_x = (f.sub_w + rays * kTile - 1) / (rays * kTile);
  if (pixel_mode == 1) {  // the status bits this launch raises are the layer's to keep
    if (hipMemsetAsync(c.pixel_status, 0, sizeof(int), s) != hipSuccess) return -1;
    g.status = c.pixel_status;
  }
  const long long tiles = tiles_y * g.tiles_x;
  long long key_tiles = 0;
  if (!ordered || trace_tile_key(f, &key_tiles) == 0 || key_tiles != tiles) {
    if (hit_mode) return -1;  // the caches are laid out for the key's grid
    g.tile_order = nullptr; g.tile_cost = nullptr; g.prev_cost = nullptr;
  }
  if (hit_mode == 2) {  // no sorter workgroup, no order, no classes
    g.tile_order = nullptr; g.tile_cost = nullptr; g.prev_cost = nullptr; g.next_order = nullptr;
  }
  // one wave per workgroup (a finished wave's slot refills at once), plus the
  // tile-order sorter (sfrt_trace.h FrameRec)
  const long long blocks = tiles + (g.prev_cost ? 1 : 0);
  if (blocks > 0x7fffffffLL) return -1;
  const dim3 gr((unsigned)blocks), b(64);
  if (f.ss < 0 || f.ss > 2 || (f.ss && dump)) return -1;  // trace_points dumps the 1x pixel
  if (f.ss && (f.sub_w | f.sub_row0 | f.sub_rows) & ((1 << f.ss) - 1)) return -1;  // whole groups
  // the cache is laid out for the ordered kernel's grid (launch_ray_fill), never dumped
  if ((ray_cache != nullptr) != (tile_recs != nullptr)) return -1;
  if (ray_cache && (!ordered || (!g.tile_cost && hit_mode != 2) || dump)) return -1;
  // the cull cache rides on the ray cache
  if ((cull_recs != nullptr) != (cull_wins != nullptr) || (cull_recs && !ray_cache)) return -1;
  // the AUX kernels compute their directions and dump nothing; one plane at least
  if (aux && (dump || ray_cache || (!aux->depth && !aux->sphere && !aux->steps))) return -1;
  // the placing kernels: row-major, their directions computed, nothing dumped; the last output
  // column's element offset fits the kernels' int
  if (place_xstride < 0 || (place_xstride && (ordered || dump || ray_cache))) return -1;
  if (place_xstride && (long long)((f.sub_w - 1) >> f.ss) * place_xstride > 0x7fffffffLL) return -1;
  const AuxArgs no_planes{};
  // The list kernels run only for n > 64: their lookahead reads culled-list lane 63, whose
  // default sphere 63 must exist (the static_assert beside first_entry).
  const bool list = f.n > kInlineSpheres;
  InlineArgs args;  // n <= 64: the frame and the records in one argument block (else unused, unset)
  if (!list) {
    args.f = g;
    for (int k = 0; k < f.n; k++) args.s[k] = host_spheres[k];
  }
  const hipEvent_t ev = (hipEvent_t)done_event;  // the record ring's slot (sfrt_world.cpp)
  // A launch of each column: the argument block, plainly; the frame record with ev as the stop
  // event; and the list dump kernel's, which records no event.
  auto inl = [&](auto k, const auto&... a) { hipLaunchKernelGGL(k, gr, b, 0, s, args, a...); };
  auto lst = [&](auto k, const auto&... a) { hipExtLaunchKernelGGL(k, gr, b, 0, s, nullptr, ev, 0, g, a...); };
  auto lst_no_event = [&](auto k, const auto&... a) { hipLaunchKernelGGL(k, gr, b, 0, s, g, a...); };
  with_rays(rays, [&](auto r) {
    with_ss(f.ss, [&](auto ss) {
      constexpr int R = decltype(r)::value, SS = decltype(ss)::value;
      // mode                n <= 64                                                 n > 64
      if (place_xstride) {
        if (aux) list ? lst(k_trace_place_list<R, SS, true>, *aux, place_xstride)
                      : inl(k_trace_place_r<R, SS, true>, *aux, place_xstride);
        else list ? lst(k_trace_place_list<R, SS, false>, no_planes, place_xstride)
                  : inl(k_trace_place_r<R, SS, false>, no_planes, place_xstride);
      } else if (aux) {
        list ? lst(k_trace_window_list_aux<R, SS>, *aux) : inl(k_trace_window_r_aux<R, SS>, *aux);
      } else if (compact_mode == 2) {
        if constexpr (SS == 0) {
          FrameRec h = g;  // the one argument (k_shade_compact): nothing of the tile order is linked
          h.tile_order = (const uint32_t*)c.compact_recs;
          h.prev_cost = (const uint8_t*)cull_recs;
          h.spheres = (const SphereRec*)c.bright_rep;
          if (list) hipExtLaunchKernelGGL(k_shade_compact<R>, gr, b, 0, s, nullptr, ev, 0, h);
          else hipLaunchKernelGGL(k_shade_compact<R>, gr, b, 0, s, h);
        }
      } else if (compact_mode == 1) {
        if constexpr (SS == 0) {
          list ? lst(k_shade_texels_cf<R>, cull_recs, (const TexelRec*)texel_recs, c.compact_recs, c.bright_rep,
                     c.bright_classes)
               : lst_no_event(k_shade_texels_cf<R>, cull_recs, (const TexelRec*)texel_recs, c.compact_recs,
                              c.bright_rep, c.bright_classes);
        }
      } else if (texel_mode == 2) {
        list ? lst(k_shade_texels<R, SS>, cull_recs, (const TexelRec*)texel_recs)
             : lst_no_event(k_shade_texels<R, SS>, cull_recs, (const TexelRec*)texel_recs);
      } else if (texel_mode == 1) {
        list ? lst(k_shade_hits_list_tf<R, SS>, cull_recs, (const HitRec*)hit_recs, texel_recs)
             : inl(k_shade_hits_tf<R, SS>, cull_recs, (const HitRec*)hit_recs, texel_recs);
      } else if (hit_mode == 2) {
        list ? lst(k_shade_hits_list<R, SS>, cull_recs, (const HitRec*)hit_recs)
             : inl(k_shade_hits<R, SS>, cull_recs, (const HitRec*)hit_recs);
      } else if (hit_mode == 1) {
        list ? lst(k_trace_window_list_hf<R, SS>, ray_cache, cull_recs, (const CullWinList*)cull_wins, hit_recs)
             : inl(k_trace_window_r_hf<R, SS>, ray_cache, cull_recs, (const CullWin*)cull_wins, hit_recs);
      } else if (cull_recs) {
        list ? lst(k_trace_window_list_cc<R, SS>, ray_cache, cull_recs, (const CullWinList*)cull_wins)
             : inl(k_trace_window_r_cc<R, SS>, ray_cache, cull_recs, (const CullWin*)cull_wins);
      } else if (ray_cache) {
        list ? lst(k_trace_window_list_rc<R, SS>, ray_cache, tile_recs)
             : inl(k_trace_window_r_rc<R, SS>, ray_cache, tile_recs);
      } else if constexpr (SS > 0) {
        list ? lst(k_trace_window_list_ss<R, SS>) : inl(k_trace_window_r_ss<R, SS>);
      } else if (dump) {
        list ? lst_no_event(k_trace_window_list_dump<R>, *dump) : inl(k_trace_window_r_dump<R>, *dump);
      } else {
        list ? lst(k_trace_window_list<R>) : inl(k_trace_window_r<R>);
      }
    });
  });
  if (hipGetLastError() != hipSuccess) return -1;
  if (pixel_mode == 1) return launch_pixels_copy<false>(f, c.pixels, c.pixel_status, s, nullptr);
  return 0;
}

void trace_views_grid(const FrameRec& f, int* tiles_x, long long* tiles) {
  const int rays = trace_rays(f, false);  // (64-bit: a width near INT_MAX must not wrap)
  *tiles_x = (int)(((long long)f.sub_w + rays * kTile - 1) / (rays * kTile));
  *tiles = (long long)*tiles_x * (((long long)f.sub_rows + kTile - 1) / kTile);
}

int launch_trace_views(const FrameRec& f, const ViewRec* dev_views, int count, bool aux,
                       void* stream, void* done_event) {
  int tiles_x = 0;
  long long tiles = 0;
  trace_views_grid(f, &tiles_x, &tiles);
  // whole frames of whole sample groups, a grid the runtime takes (work-items per dimension in 32
  // bits, views in the y dimension's 16), the table's tiles_x this kernel's
  if (!dev_views || count <= 0 || count > 0xffff || f.n <= 0 || !f.spheres || f.ss < 0 || f.ss > 2) return -1;
  if (tiles <= 0 || tiles * 64 > 0xffffffffLL || tiles * count > 0x7fffffffLL || f.tiles_x != tiles_x) return -1;
  if (f.sub_row0 != 0 || (f.ss && (f.sub_w | f.sub_rows) & ((1 << f.ss) - 1))) return -1;
  const dim3 gr((unsigned)tiles, (unsigned)count), b(64);
  hipStream_t s = (hipStream_t)stream;
  const hipEvent_t ev = (hipEvent_t)done_event;
  const bool list = f.n > kInlineSpheres;  // as launch_trace
  auto go = [&](auto k) { hipExtLaunchKernelGGL(k, gr, b, 0, s, nullptr, ev, 0, dev_views); };
  with_rays(trace_rays(f, false), [&](auto r) {
    with_ss(f.ss, [&](auto ss) {
      constexpr int R = decltype(r)::value, SS = decltype(ss)::value;
      if (aux) list ? go(k_trace_views<R, SS, true, true>) : go(k_trace_views<R, SS, false, true>);
      else list ? go(k_trace_views<R, SS, true, false>) : go(k_trace_views<R, SS, false, false>);
    });
  });
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace {

template <bool SHADE, bool OWN>
void launch_cast(const FrameRec& f, const SphereRec* host_spheres, const RayArgs& rays, dim3 gr,
                 hipStream_t s, hipEvent_t ev) {
  const dim3 b(64);
  if (f.n <= kInlineSpheres) {
    InlineArgs args;
    args.f = f;
    for (int k = 0; k < f.n; k++) args.s[k] = host_spheres[k];
    hipLaunchKernelGGL((k_cast_rays<false, SHADE, OWN>), gr, b, 0, s, args, rays);
  } else {
    hipExtLaunchKernelGGL((k_cast_rays<true, SHADE, OWN>), gr, b, 0, s, nullptr, ev, 0, f, rays);
  }
}

}  // namespace

int launch_cast_rays(const FrameRec& f, const SphereRec* host_spheres, const RayArgs& rays,
                     void* stream, void* done_event) {
  if (rays.count <= 0 || rays.count > 0x7fffffffLL || !rays.dirs || f.n <= 0) return -1;
  if (!rays.pos && !rays.depth && !rays.sphere && !rays.steps && !rays.rgba) return -1;
  if (f.n > kInlineSpheres && !f.spheres) return -1;
  const dim3 gr((unsigned)((rays.count + 63) / 64));
  hipStream_t s = (hipStream_t)stream;
  const hipEvent_t ev = (hipEvent_t)done_event;
  const bool own = rays.origins != nullptr;
  if (rays.rgba) {
    if (own) launch_cast<true, true>(f, host_spheres, rays, gr, s, ev);
    else launch_cast<true, false>(f, host_spheres, rays, gr, s, ev);
  } else {
    if (own) launch_cast<false, true>(f, host_spheres, rays, gr, s, ev);
    else launch_cast<false, false>(f, host_spheres, rays, gr, s, ev);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sfrt
