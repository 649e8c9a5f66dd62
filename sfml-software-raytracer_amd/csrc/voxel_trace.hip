// voxel_trace.hip -- gfx950 kernel for the reference's voxel World frame fill
// (SURVEY 8f row f2): World::Raycast / World::LRaycast,
// /root/reference/Raytracing/World.cpp:302-491, one lane per pixel.
//
// Bit-exact with oracle/voxelworld_oracle.c: binary32 in the reference's
// expression order, -ffp-contract=off, correctly rounded division and sqrt,
// and the x86-64 float->integer conversions of the reference's build
// (out-of-range and NaN give INT_MIN / 0) emulated explicitly.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "sfrt_device.h"
#include "sfrt_math.h"
#include "voxel_trace.h"

#pragma clang fp contract(off)

// cell_hit's buffer descriptor word 3 (0x00020000, DATA_FORMAT_32) is the gfx9 / CDNA encoding;
// gfx10+ lay that word out differently.  This file is built for gfx950 only.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "voxel_trace.hip: the grid's buffer descriptor is encoded for gfx950 (CDNA4)"
#endif

namespace sfrt {
namespace {

constexpr float kPI = 3.1415926535f;     // World.h:5
constexpr float kPI2 = 6.28318530718f;   // World.h:6

// x86-64 cvttss2si semantics (the reference's build): INT_MIN when out of range or NaN.
__device__ __forceinline__ int32_t to_i32(float f) {
  return (f > -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : (int32_t)0x80000000;
}
// A primary-ray DDA position to its cell coordinate: to_i32, or in the fast DDA (every lane of
// the wave within the host's dda_qlim bound, so |f| < 2^30) the plain conversion it equals
// there -- one v_cvt_i32_f32 instead of a compare, a conversion and a select per axis and step.
// FAST is raycast_t's parameter of that name: a property of the wave's positions, proved by
// whoever picks the instantiation (raycast() from the frame's dda_qlim, the ray batches from
// the wave's own origins and directions, walk_bounded), and not of the divisions (RECIP).
template <bool FAST>
__device__ __forceinline__ int32_t pos_i32(float f) {
  return FAST ? (int32_t)f : to_i32(f);
}
// float -> unsigned as x86-64 g++ emits it: 64-bit cvttss2si, low 32 bits.
__device__ __forceinline__ uint32_t to_u32(float f) {
  if (!(f > -9.2233720368547758e18f && f < 9.2233720368547758e18f)) return 0u;
  return (uint32_t)(long long)f;
}
__device__ __forceinline__ uint32_t to_u8(float f) {
  return (uint32_t)to_i32(f) & 0xffu;
}
__device__ __forceinline__ float min255(float v) { return 255.0f < v ? 255.0f : v; }

struct V3 {
  float x, y, z;
};

// blocks.contains((x << 20) + (y << 10) + z) (World.cpp:385, 476).  The reference's map key IS
// a linear index: (x << 20) + (y << 10) + z, in wrapping 32-bit arithmetic, is the offset of cell
// (x, y, z) in a dense [2048][1024][1024] array, and every stored key lies below nx << 20.  So the
// host stores the world as that array of bytes (VoxFrame::cells, nx << 20 bytes: code = id +
// kVoxCellBias, 0 = empty; rows and planes beyond ny / nz stay 0), and a lookup is the key itself
// as the byte offset of a buffer load whose range check (num_records = nx << 20) returns 0 for
// every key at or past the last x-plane -- negative keys included (>= 2^31 as unsigned).  No
// decode of the key, no validity compares, no index arithmetic: two v_lshl_add_u32 and the load
// per step, exactly the reference's contains() (profiles/ab/r5_ab1).  `code` is the cell's code
// when the cell is hit (id = code - kVoxCellBias).
__device__ __forceinline__ bool cell_hit(const VoxFrame& f, int32_t x, int32_t y, int32_t z,
                                         uint32_t& code) {
  // ((x << 10) + y) << 10) + z: two v_lshl_add_u32 (left alone: two shifts and an add3)
  uint32_t key;
  __asm__("v_lshl_add_u32 %0, %1, 10, %2" : "=v"(key) : "v"(x), "v"(y));
  __asm__("v_lshl_add_u32 %0, %1, 10, %2" : "=v"(key) : "v"(key), "v"(z));
  const __amdgpu_buffer_rsrc_t cells =
      __builtin_amdgcn_make_buffer_rsrc((void*)f.cells, (short)0, (int)f.cell_bytes, 0x00020000);
  code = __builtin_amdgcn_raw_buffer_load_b8(cells, (int)key, 0, 0);
  return code != 0u;
}

__device__ __forceinline__ uint32_t texel(const VoxFrame& f, const VoxTex& t, uint32_t x,
                                          uint32_t y) {
  const uint32_t idx = x + y * (uint32_t)t.w;
  if (t.texels == nullptr || idx >= (uint32_t)(t.w * t.h)) {
    atomicOr(f.status, 2);       // the reference reads outside the image here
    return 0xffff00ffu;          // magenta, as the oracle
  }
  return t.texels[idx];
}

// The DDA divides by the same |dir| components at every step.  With their
// correctly rounded reciprocals, sfrt_math::div_recip gives the same bits as
// the division for b in [2^-60, 2^60]; a wave with any lane
// outside that range (an axis-parallel ray has |dir.x| == 0) divides plainly.
__device__ __forceinline__ bool recip_ok(float b) { return b >= 0x1.0p-60f && b <= 0x1.0p60f; }

// dirXadd + sign * (pos - (float)ipos) (World.cpp:330-332, 466-468): sign is +-1, so the product
// is exact and one fma rounds the sum exactly as the reference's add does (NaN and inf alike).
__device__ __forceinline__ float dda_num(float add, float sign, float p, int32_t ip) {
  return __builtin_fmaf(sign, p - (float)ip, add);
}

template <bool RECIP>
__device__ __forceinline__ float dv(float a, float b, float y) {
  return RECIP ? sfrt_math::div_recip(a, b, y) : a / b;
}

// Light j through the constant address space (the table is never written by a launch):
// the wave-uniform loads become scalar loads instead of vector loads into VGPRs.
__device__ __forceinline__ VoxLight light_at(const VoxLight* p, int j) {
  const __attribute__((address_space(4))) uint32_t* q =
      (const __attribute__((address_space(4))) uint32_t*)(p + j);
  uint32_t w[sizeof(VoxLight) / 4];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(VoxLight) / 4); i++) w[i] = q[i];
  VoxLight l;
  __builtin_memcpy(&l, w, sizeof l);
  return l;
}

__device__ __forceinline__ uint32_t pack(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
  return r | (g << 8) | (b << 16) | (a << 24);
}

// World::LRaycast, World.cpp:455-491.
template <bool RECIP>
__device__ bool lraycast_t(const VoxFrame& f, V3 pos, V3 dir, float maxDist,
                           uint32_t& work) {
  float dist = 0.0f;
  int32_t pix = to_i32(pos.x), piy = to_i32(pos.y), piz = to_i32(pos.z);
  const float dirxadd = dir.x > 0 ? 1.0f : 0.0f, diryadd = dir.y > 0 ? 1.0f : 0.0f,
              dirzadd = dir.z > 0 ? 1.0f : 0.0f;
  const float sx = dir.x > 0 ? -1.0f : 1.0f, sy = dir.y > 0 ? -1.0f : 1.0f,
              sz = dir.z > 0 ? -1.0f : 1.0f;
  const float lx = fabsf(dir.x), ly = fabsf(dir.y), lz = fabsf(dir.z);
  const float yx = RECIP ? 1.0f / lx : 0.0f, yy = RECIP ? 1.0f / ly : 0.0f,
              yz = RECIP ? 1.0f / lz : 0.0f;
  const float m2 = maxDist * 2;
  const uint32_t maxIter = to_u32(m2 < 20.0f ? 20.0f : m2);
  // One way out of the loop, as in raycast_t: the reference's loop test and its block hit
  // (return false) become one stop condition at the bottom of the step, the cell of the next
  // step's top tested there (only while the loop test holds, as the reference tests it).
  bool blocked = false;
  if ((0u < maxIter) & (dist < maxDist)) {
    work++;
    uint32_t code;
    blocked = cell_hit(f, pix, piy, piz, code);
    if (!blocked) {
      for (uint32_t i = 0;;) {
        const float a = dv<RECIP>(dda_num(dirxadd, sx, pos.x, pix), lx, yx);
        const float b = dv<RECIP>(dda_num(diryadd, sy, pos.y, piy), ly, yy);
        const float c = dv<RECIP>(dda_num(dirzadd, sz, pos.z, piz), lz, yz);
        float raySpeed = a;  // std::min({a, b, c})
        if (b < raySpeed) raySpeed = b;
        if (c < raySpeed) raySpeed = c;
        raySpeed += 0.002f;
        dist += raySpeed;
        pos.x = pos.x + dir.x * raySpeed;
        pos.y = pos.y + dir.y * raySpeed;
        pos.z = pos.z + dir.z * raySpeed;
        pix = to_i32(pos.x); piy = to_i32(pos.y); piz = to_i32(pos.z);
        i++;
        const bool more = (i < maxIter) & (dist < maxDist);
        work += more ? 1u : 0u;
        blocked = more & cell_hit(f, pix, piy, piz, code);
        if (!more | blocked) break;
      }
    }
  }
  return !blocked & (dist >= maxDist);
}

__device__ bool lraycast(const VoxFrame& f, V3 pos, V3 dir, float maxDist,
                         uint32_t& work) {
  const bool ok = recip_ok(fabsf(dir.x)) && recip_ok(fabsf(dir.y)) && recip_ok(fabsf(dir.z));
  if (__builtin_amdgcn_ballot_w64(!ok)) return lraycast_t<false>(f, pos, dir, maxDist, work);
  return lraycast_t<true>(f, pos, dir, maxDist, work);
}

// The hit block of World::Raycast (World.cpp:385-450): texel of the face the step crossed,
// light from every light source with shadow rays.  `dist` is the step's tryDist.
template <bool RECIP>
__device__ __forceinline__ uint32_t shade_hit(const VoxFrame& f, V3 pos, int32_t pix, int32_t piy,
                                              int32_t piz, int colRay, float sx, float sy,
                                              float sz, float dist, int id, uint32_t& work) {
  uint32_t c;
  if (id < 0) {
    c = f.colors[-id];
  } else {
    // the reference's three face branches (World.cpp:395-412) as selects of the same
    // expressions: one texel fetch per lane whatever mix of faces the wave's lanes hit
    const VoxTex& t = f.tex[id];
    const float tw = (float)(uint32_t)t.w, th = (float)(uint32_t)t.h;
    const float fx = pos.x - (float)pix, fy = pos.y - (float)piy, fz = pos.z - (float)piz;
    const bool c1 = colRay == 1, c2 = colRay == 2, c3 = !c1 & !c2;
    c = texel(f, t, to_u32(tw * (c1 ? fz : fx)), to_u32(th * (c2 ? fz : fy)));
    pos.x = c1 ? pos.x + sx * 0.01f : pos.x;  // get it off the wall
    pos.y = c2 ? pos.y + sy * 0.01f : pos.y;
    pos.z = c3 ? pos.z + sz * 0.01f : pos.z;
    sx = c1 ? sx : 0.0f;
    sy = c2 ? sy : 0.0f;
    sz = c3 ? sz : 0.0f;
  }
  const float l0 = 0.05f / dist - dist * 0.0001f;
  float litr = l0 < 0.0f ? 0.0f : l0;
  float litg = litr, litb = litr;
  // the record address stepped (a j * 36 product per light was four scalar instructions) and
  // the skip test's fields one scalar load (VoxLight): 4K 201.5 -> 198.0 us (profiles/ab/r5_ab2)
  const VoxLight* const lend = f.lights + f.nlights;
  for (const VoxLight* lp = f.lights; lp != lend; ++lp) {
    const VoxLight L = light_at(lp, 0);
    const float ex = pos.x - L.px, ey = pos.y - L.py, ez = pos.z - L.pz;
    // dd >= dd_pass: the light adds nothing (host threshold, exact); a wave none of whose lanes
    // is that close skips the light's division and the rest.  The test is ours: the squared
    // distance by two fmas against the host's inflated dd_skip (voxel_trace.h), and the body
    // evaluates the reference's dd
    const float ddf = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
    if (!__builtin_amdgcn_ballot_w64(ddf < L.dd_skip)) continue;
    float dd = ex * ex + ey * ey + ez * ez;  // VLengthS
    float add = (L.intensity / dd - dd * 0.002f);
    if (add > 0) {
      float nx = L.px - pos.x, ny = L.py - pos.y, nz = L.pz - pos.z;
      add *= ((nx * sx + ny * sy + nz * sz) * 0.7f + 0.3f);
      if (add > 0) {
        bool lit = true;
        if (L.shadows && dist < f.shadow_distance) {
          dd = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);  // VLength
          nx = nx / dd; ny = ny / dd; nz = nz / dd;
          lit = lraycast(f, pos, V3{nx, ny, nz}, dd, work);
        }
        if (lit) {
          litr += add * L.r;
          litg += add * L.g;
          litb += add * L.b;
        }
      }
    }
  }
  return pack(to_u8(min255((float)(c & 0xffu) * litr)),
              to_u8(min255((float)((c >> 8) & 0xffu) * litg)),
              to_u8(min255((float)((c >> 16) & 0xffu) * litb)), c >> 24);
}

// What ended World::Raycast for the lane (AUX kernels; include/sfrt.h "the voxel frame fill's
// per-pixel planes"): read after the step loop from the registers the loop carries anyway.
struct VoxHit {
  float depth;
  int32_t cell, face, steps;
};

// What a ray batch (k_voxel_cast_rays) adds to a lane's ray: whether the lane marches at all (a
// lane past the batch's end or with an invalid ray does not enter the step loop), the ray's own
// origin (OWN) and, back, r->pos where Raycast ended.  The frame kernels pass none (NoRay).
struct BatchRay {
  bool live;
  V3 org;
  V3 end;
};
struct NoRay {};

// World::Raycast, World.cpp:302-453.  AUX: also the outcome in `hit` (untouched without it).
// RECIP: the reciprocal divisions (every lane's |dir| components within recip_ok).  FAST: the
// plain position conversions and the NaN-free choice of the step's axis -- every position of
// every lane's walk stays below 2^30 in magnitude (pos_i32).  FAST implies RECIP's operands are
// finite with normal or zero quotients; RECIP without FAST is not instantiated (a position past
// 2^31 makes numerators that overflow the quotient, where div_recip gives NaN for the division's
// inf).  The ray batches (RAY = BatchRay) add: OWN, the ray starts at its own origin and the
// billboard list is not visited; SHADE = false, a block hit is not shaded (returns 0).
// VIEW: where the per-camera fields are read -- the camera and the billboard table here, dda_qlim
// in raycast(), the col / row tables, the target and the tile-order pointers in voxel_tile.  The
// frame itself everywhere but in the view batches (k_voxel_views), whose waves take them from
// their view's record (VoxViewRec); every other field is f's.  (A modified copy of the frame
// would not do: the texture and colour tables are indexed per lane, in the kernel's arguments
// that is a load, in a copy it is 552 bytes of scratch.)
template <bool RECIP, bool FAST, bool AUX, bool OWN = false, bool SHADE = true, class RAY = NoRay,
          class VIEW = VoxFrame>
__device__ uint32_t raycast_t(const VoxFrame& f, const VIEW& v, V3 dir, float yscale,
                              float atan_dir, uint32_t& work, VoxHit& hit, RAY& ray) {
  static_assert(RECIP == FAST, "the reciprocal divisions are proved under FAST's bound only");
  constexpr bool BATCH = !__is_same(RAY, NoRay);
  static_assert(BATCH || (!OWN && SHADE), "OWN and SHADE = false are the ray batches'");
  const V3 cam{v.cam[0], v.cam[1], v.cam[2]};
  float dist = 0.0f;
  V3 pos = cam;
  if constexpr (OWN) pos = ray.org;
  int32_t pix = pos_i32<FAST>(pos.x), piy = pos_i32<FAST>(pos.y), piz = pos_i32<FAST>(pos.z);
  // The reference's tryPos (World.cpp:318) equals pos at the top of every step (pos = tryPos
  // ends each step), so the step advances pos in place after the billboard loop, which works
  // on copies of pos and dist (the reference moves both there and then overwrites them with
  // tryPos / tryDist): no second position carried around the loop and copied back each step.
  const float dirxadd = dir.x > 0 ? 1.0f : 0.0f, diryadd = dir.y > 0 ? 1.0f : 0.0f,
              dirzadd = dir.z > 0 ? 1.0f : 0.0f;
  const float sx = dir.x > 0 ? -1.0f : 1.0f, sy = dir.y > 0 ? -1.0f : 1.0f,
              sz = dir.z > 0 ? -1.0f : 1.0f;   // dir*sign (short, exact as float)
  const float lx = fabsf(dir.x), ly = fabsf(dir.y), lz = fabsf(dir.z);
  const float yx = RECIP ? 1.0f / lx : 0.0f, yy = RECIP ? 1.0f / ly : 0.0f,
              yz = RECIP ? 1.0f / lz : 0.0f;
  int DI = 0;
  float dnext = f.ndyn > 0 ? v.dyn[0].dist : __builtin_nanf("");  // next billboard; NaN: never >=
  if constexpr (OWN) dnext = __builtin_nanf("");  // no billboard: f.dyn is not read
  int colRay = 0;
  float last_x = 0.0f, last_y = 0.0f, last_z = 0.0f;  // the last step's rays (colRay, below)
  // Shading after the loop: a lane that hits a block (or a billboard's opaque texel) stops
  // stepping, and the wave shades all its hit lanes once, after its last lane has stopped.
  // Shaded inside the loop, the light loop and its shadow rays ran once per distinct hit step
  // of the wave with the lanes of that step only (profiles/ab/r4_ab7: 4K 299 -> 289 us; with
  // the per-wave light skip 265 us).
  //
  //
  // One way out of the step loop: the reference leaves World::Raycast's loop three ways (its
  // loop test, a block hit, a billboard's opaque texel); as three divergent exits the compiler
  // kept a lane mask per exit and merged EXEC around each, ~35 scalar instructions and 3
  // branches per step (tools/isa_block_profile.py).  Here a lane tests one stop condition at the
  // bottom of the step, and what stopped it is read from registers afterwards: `early` != 0 (a
  // billboard's texel, alpha > 127), else `hcode` != 0 (the cell code of a block), else it marched
  // out.  A billboard's texel stops its lane through the loop test (the step's distance made
  // +inf); the lane still advances in that step, and nothing of it but `early` is read afterwards.
  // The first loop test is uniform (dist = 0, i = 0).  4K 234.6 -> 208.7 us, and 208.0 -> 201.5
  // with the outcome read back this way and the axis choice kept out of the loop's lane masks
  // (profiles/ab/r5_ab1, r5_ab2); with the two-instruction key, the billboard stop through the
  // distance and the step counters compiled out when no tile cost is recorded (k_voxel_ordered
  // COST): 200.8 -> 192.3 us (r5_ab4).  The hit face's axis (colRay) is recomputed after the loop
  // from the lane's last step's rays, by the step's own rule: computed in the loop it cost two
  // selects per step, and left for the compiler to sink it carried two lane masks merged with
  // EXEC every step (193.3 -> 188.0 us, r5_ab6).
  uint32_t hcode = 0u, early = 0u;
  // AUX: the trips of the loop's body (the one that hit included), and the distance of the
  // billboard that stopped the lane (its `dist` is +inf by then; DI stays at that billboard)
  uint32_t trips = 0u;
  float stop_dist = 0.0f;
  V3 stop_pos{0.0f, 0.0f, 0.0f};  // BATCH: the position of that billboard (bp; pos moves on)
  if (0.0f < f.view_distance && 0u < f.maxiter) {
    if constexpr (BATCH) {  // a lane without a ray to march stays out of the step loop
      if (!ray.live) goto marched;
    }
    for (uint32_t i = 0;;) {
      work++;
      const float xray = dv<RECIP>(dda_num(dirxadd, sx, pos.x, pix), lx, yx);
      const float yray = dv<RECIP>(dda_num(diryadd, sy, pos.y, piy), ly, yy);
      const float zray = dv<RECIP>(dda_num(dirzadd, sz, pos.z, piz), lz, yz);
      // the reference's if / else-if / else (World.cpp:330-350) as selects: one branch-free
      // step.  In the fast DDA no ray is NaN (finite numerators over |d| >= 2^-60), so the
      // reference's choice is the first axis whose ray equals the minimum (v_min3_f32; +-0
      // compare equal).  The speed can differ from the reference's only in the sign of a zero (a
      // negative ray underflowing to -0 beside a +0 one), which reaches the position only through
      // dir * speed added to a -0.0 component (a -0.0 camera coordinate not yet moved), and no
      // output depends on that sign (to_i32, the fractions, the texel and light offsets all map
      // +-0 alike)
      bool ax, ay;
      float raySpeed;
      if (FAST) {
        raySpeed = fminf(fminf(xray, yray), zray);
        ax = xray == raySpeed;
        ay = !ax & (yray == raySpeed);
      } else {
        ax = (xray <= yray) & (xray <= zray);
        ay = !ax & (yray <= xray) & (yray <= zray);
        raySpeed = ax ? xray : (ay ? yray : zray);
      }
      const float rs2 = raySpeed + 0.002f;
      last_x = xray; last_y = yray; last_z = zray;
      float tryDist = dist + raySpeed;
      // dynamic billboards in front of the next block (World.cpp:353-378): the next billboard's
      // distance is held in a register (NaN past the last), so the test reads no memory on the
      // steps that pass no billboard (nearly all), and a wave whose lanes all pass none skips
      // the loop, which works on copies of pos and dist (the reference moves both there and then
      // overwrites them with tryPos / tryDist)
      if (__builtin_amdgcn_ballot_w64(tryDist >= dnext)) {
        V3 bp = pos;
        float bdist = dist;
        while (tryDist >= dnext) {
          const VoxDyn& d = v.dyn[DI];
          const float bs = d.dist - bdist;
          bdist = d.dist;
          bp.x = bp.x + dir.x * bs;
          bp.y = bp.y + dir.y * bs;
          bp.z = bp.z + dir.z * bs;
          const float to = d.py - bp.y;
          const float sizey = d.sy * yscale;
          if (fabsf(to) < sizey) {
            float ang = d.atan_b - atan_dir;  // VAngleXZ(dir, VNormalizeXZ(d->pos - cam.pos))
            ang = ang > kPI ? ang - kPI2 : (ang < -kPI ? ang + kPI2 : ang);
            ang = ang * bdist;
            const VoxTex& t = f.dyn_tex[d.tex];
            const float xf = (0.5f + ang / kPI * 0.5f / d.sx);
            if (xf > 0 && xf < 1) {
              int32_t x = to_i32(xf * (float)(uint32_t)t.w);
              int32_t y = to_i32((sizey + to) / sizey / 2 * (float)(uint32_t)t.h);
              x = x < 0 ? 0 : x;
              y = y < 0 ? 0 : y;
              const uint32_t c = texel(f, t, (uint32_t)x, (uint32_t)y);
              if ((c >> 24) > 127u) {
                early = pack(to_u8(min255((float)(c & 0xffu) * d.r)),
                             to_u8(min255((float)((c >> 8) & 0xffu) * d.g)),
                             to_u8(min255((float)((c >> 16) & 0xffu) * d.b)), c >> 24);
                tryDist = __builtin_inff();  // stops the lane through the loop test
                if constexpr (AUX) stop_dist = bdist;
                if constexpr (BATCH) stop_pos = bp;
                break;
              }
            }
          }
          DI++;
          dnext = DI < f.ndyn ? v.dyn[DI].dist : __builtin_nanf("");
        }
      }
      dist = tryDist;
      pos.x += dir.x * (ax ? rs2 : raySpeed);  // tryPos (World.cpp:330-350)
      pos.y += dir.y * (ay ? rs2 : raySpeed);
      pos.z += dir.z * ((ax | ay) ? raySpeed : rs2);
      pix = pos_i32<FAST>(pos.x); piy = pos_i32<FAST>(pos.y); piz = pos_i32<FAST>(pos.z);
      cell_hit(f, pix, piy, piz, hcode);  // hcode != 0: hit a block (World.cpp:385)
      i++;
      if constexpr (AUX) trips = i;
      if ((hcode != 0u) | !(dist < f.view_distance) | !(i < f.maxiter)) break;
    }
  }
marched:
  if constexpr (AUX) {  // a march-out; the two returns below overwrite their fields
    hit.depth = dist;
    hit.cell = -1;
    hit.face = 0;
    hit.steps = (int32_t)trips;
  }
  if constexpr (BATCH) ray.end = early != 0u ? stop_pos : pos;  // :357, or :381 / the loop's exit
  if (early != 0u) {  // a billboard's texel with alpha > 127: never 0
    if constexpr (AUX) {
      hit.depth = stop_dist;
      hit.cell = DI;
      hit.face = 4;
    }
    return early;
  }
  // the axis of the lane's last step, from that step's rays (kept in registers: the loop's last
  // assignment is its exit value), by the step's own rule
  if (FAST) {
    const float rs = fminf(fminf(last_x, last_y), last_z);
    colRay = last_x == rs ? 1 : (last_y == rs ? 2 : 3);
  } else {
    const bool ax = (last_x <= last_y) & (last_x <= last_z);
    const bool ay = !ax & (last_y <= last_x) & (last_y <= last_z);
    colRay = ax ? 1 : (ay ? 2 : 3);
  }
  if (hcode != 0u) {
    if constexpr (AUX) {
      // the key of the lookup that hit (World.cpp:385, wrapping), and the crossed face: the axis
      // with the sign of dirXsign (World.cpp:312-314), the face's outward normal
      hit.cell = (int32_t)(((uint32_t)pix << 20) + ((uint32_t)piy << 10) + (uint32_t)piz);
      hit.face = colRay == 1 ? (sx < 0.0f ? -1 : 1) : colRay == 2 ? (sy < 0.0f ? -2 : 2)
                                                                  : (sz < 0.0f ? -3 : 3);
    }
    if constexpr (!SHADE) return 0u;  // the picking path: no texel, no light loop, no shadow rays
    return shade_hit<RECIP>(f, pos, pix, piy, piz, colRay, sx, sy, sz, dist,
                            (int)hcode - kVoxCellBias, work);
  }
  return pack(0, 0, 0, 255);  // sf::Color::Black
}

template <bool AUX, class VIEW>
__device__ uint32_t raycast(const VoxFrame& f, const VIEW& v, V3 dir, float yscale,
                            float atan_dir, uint32_t& work, VoxHit& hit) {
  // the reciprocal divisions and, within the host's bound on the direction's spread, the plain
  // position conversions (pos_i32)
  const float lx = fabsf(dir.x), ly = fabsf(dir.y), lz = fabsf(dir.z);
  const bool ok = recip_ok(lx) && recip_ok(ly) && recip_ok(lz) &&
                  fmaxf(fmaxf(lx, ly), lz) <= v.dda_qlim * fminf(fminf(lx, ly), lz);
  NoRay none;
  if (__builtin_amdgcn_ballot_w64(!ok))
    return raycast_t<false, false, AUX>(f, v, dir, yscale, atan_dir, work, hit, none);
  return raycast_t<true, true, AUX>(f, v, dir, yscale, atan_dir, work, hit, none);
}

// The lane's outcome into the planes of `aux` at output pixel (row r, column a) of the band.
__device__ __forceinline__ void store_planes(const VoxAux& aux, const VoxHit& hit, int r, int a) {
  if (aux.depth) aux.depth[(long long)r * aux.depth_pitch + a] = hit.depth;
  if (aux.cell) aux.cell[(long long)r * aux.cell_pitch + a] = hit.cell;
  if (aux.face) aux.face[(long long)r * aux.face_pitch + a] = hit.face;
  if (aux.steps) aux.steps[(long long)r * aux.steps_pitch + a] = hit.steps;
}

// 8x8 pixels per one-wave workgroup (a finished wave's slot refills at once;
// 0.7-1.5% faster than 16x16 per 256 threads).
// The default: 8x8 tiles on a 1-D grid of one-wave workgroups in the adaptive
// tile order (sfrt_device.h sort_tiles; workgroup 0 is the sorter when
// prev_cost is set).
// Eight waves per SIMD: 58 VGPRs since the shading left the DDA loop (72 before, seven waves).
#ifndef SFRT_VOX_WAVES
#define SFRT_VOX_WAVES 8
#endif
// SS (SFRT_OPT_SUPERSAMPLE, S = 1 << SS = 2 or 4): the tile is of samples -- the pixels of
// World::UpdateImage at S * width x S * height, f's subset, tables and strides in samples (the
// host, sfrt_voxel.cpp) -- traced and shaded as always, then box-filtered over each S x S group of
// lanes (sfrt_device.h group_box_rgba8) into the one output pixel its leader lane stores.  The
// subset's width and rows are multiples of S and tiles start at multiples of 8, so a group is
// wholly inside the subset or wholly clamped duplicates, and the adds cross no group.  The order,
// the sorter, the fast-DDA choice and the cost record run on the sample grid unchanged.
//
// voxel_tile is the workgroup's part of the launch up to the tile's stores: false for the sorter,
// else the tile, its class in the order (sfrt_device.h slot_tile) and its lanes' step counts.  The
// cost record that follows stays in the kernels' own bodies: inlined through here the compiler
// turned tile_bucket's chain into other scalar code, and k_voxel_ordered<true> is to compile to
// what it did before the supersampling kernels came.
//
// AUX (k_voxel_aux): the planes of `aux` beside the colour, one dword per non-null plane from the
// lane that stores the pixel -- for SS > 0 the group's leader, whose sample is the output pixel's
// first, (S * i, S * j).  The null tests are wave-uniform (kernel arguments).
//
// PLACE (k_voxel_place; sfrt_voxel_render_subset): the subset in place in a whole frame -- output
// column a is stored xstride elements apart, the host having put the subset's first pixel into
// f.out and yadd frame rows into f.out_pitch (the planes' pitches likewise).
template <int SS, bool AUX, bool PLACE = false, class VIEW>
__device__ __forceinline__ bool voxel_tile(const VoxFrame& f, const VIEW& v, const VoxAux& aux, int tiles_x,
                                           int ntiles, int& tile, uint32_t& cls, uint32_t& work,
                                           [[maybe_unused]] int xstride = 1) {
  const int lane = threadIdx.x & 63;
  int slot = (int)blockIdx.x;
  if (v.prev_cost) {
    if (slot == 0) {
      sort_tiles(f.prev_cost, ntiles, f.next_order);
      return false;
    }
    slot -= 1;
  }
  tile = slot_tile(v.tile_order, slot, ntiles, cls);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int a = tx * 8 + (lane & 7);
  const int b = f.sub_row0 + ty * 8 + (lane >> 3);
  // Edge lanes trace a clamped duplicate pixel and store nothing (a divergent
  // branch around raycast() would make its wave-uniform choices divergent).
  const int ac = a < f.sub_w ? a : f.sub_w - 1;
  const int bc = b < f.sub_row0 + f.sub_rows ? b : f.sub_row0 + f.sub_rows - 1;
  const int i = subset_index<SS>(f.xstart, f.xadd, ac);
  const int j = subset_index<SS>(f.ystart, f.yadd, bc);
  work = 0;
  const V3 dir{v.col[3 * i], v.row[2 * j], v.col[3 * i + 1]};
  VoxHit hit;
  const uint32_t rgba = raycast<AUX>(f, v, dir, v.row[2 * j + 1], v.col[3 * i + 2], work, hit);
  // The store's pixel from the lane id again (mbcnt, not threadIdx): kept live across
  // raycast(), a, b and `in` were spilled to scratch (16 bytes per lane).
  const int lane2 = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int a2 = tx * 8 + (lane2 & 7), r2 = ty * 8 + (lane2 >> 3);
  if constexpr (PLACE) {
    // as the two branches below, the output column xstride elements apart (< 2^31: the host)
    const int c2 = (a2 >> SS) * xstride;
    uint32_t px = rgba;
    bool store = a2 < f.sub_w && r2 < f.sub_rows;
    if constexpr (SS > 0) {
      px = group_box_rgba8<SS>(rgba);
      store = store && group_leader<SS>(lane2);
    }
    if (store) {
      v.out[(long long)(r2 >> SS) * f.out_pitch + c2] = px;
      if constexpr (AUX) store_planes(aux, hit, r2 >> SS, c2);
    }
  } else if constexpr (SS == 0) {
    if (a2 < f.sub_w && r2 < f.sub_rows) {
      v.out[(long long)r2 * f.out_pitch + a2] = rgba;
      if constexpr (AUX) store_planes(aux, hit, r2, a2);
    }
  } else {
    // every lane has its sample (edge lanes their duplicates) and the wave has reconverged
    // (raycast()'s branches are wave-uniform): the output pixel of sample (a2, r2) of the band is
    // (a2 >> SS, r2 >> SS), out and its pitch in output pixels
    const uint32_t px = group_box_rgba8<SS>(rgba);
    if (group_leader<SS>(lane2) && a2 < f.sub_w && r2 < f.sub_rows) {
      v.out[(long long)(r2 >> SS) * f.out_pitch + (a2 >> SS)] = px;
      if constexpr (AUX) store_planes(aux, hit, r2 >> SS, a2 >> SS);
    }
  }
  return true;
}

// COST: record the tile's cost for the adaptive order (f.tile_cost set); without it the step
// counters are dead code and compiled out (one VALU per DDA and shadow-ray step)
template <bool COST>
__global__ __launch_bounds__(64, SFRT_VOX_WAVES) void k_voxel_ordered(VoxFrame f, int tiles_x, int ntiles) {
  int tile;
  uint32_t cls, work;
  if (!voxel_tile<0, false>(f, f, VoxAux{}, tiles_x, ntiles, tile, cls, work)) return;
  if (COST) {
    // the tile's slowest ray, in DDA + shadow steps / 4 (the classes' scale)
    const uint32_t w = wave_max_u32(work);
    if ((threadIdx.x & 63) == 0) store_cost(f.tile_cost, tile, tile_bucket(w >> 2), cls, f.cost_diff);
  }
}
// The supersampling instantiations (SS = 1, 2), kernels of their own: k_voxel_ordered compiles to
// what it did without them.
template <bool COST, int SS>
__global__ __launch_bounds__(64, SFRT_VOX_WAVES) void k_voxel_ordered_ss(VoxFrame f, int tiles_x, int ntiles) {
  int tile;
  uint32_t cls, work;
  if (!voxel_tile<SS, false>(f, f, VoxAux{}, tiles_x, ntiles, tile, cls, work)) return;
  if (COST) {  // as k_voxel_ordered: the sample tile's slowest ray
    const uint32_t w = wave_max_u32(work);
    if ((threadIdx.x & 63) == 0) store_cost(f.tile_cost, tile, tile_bucket(w >> 2), cls, f.cost_diff);
  }
}

// The plane-writing instantiations (sfrt_voxel_render_band_aux), kernels of their
// own over COST x SS with the planes in a kernel argument of their own: the kernels above keep
// their arguments and compile to what they did.  The outcome's registers stay live across the
// shading, so these take a bound of their own, seven waves per SIMD (up to 72 VGPRs): 63 VGPRs and
// still eight waves without the cost record, 67 and seven with it, no scratch.
#ifndef SFRT_VOX_AUX_WAVES
#define SFRT_VOX_AUX_WAVES 7
#endif
template <bool COST, int SS>
__global__ __launch_bounds__(64, SFRT_VOX_AUX_WAVES) void k_voxel_aux(VoxFrame f, int tiles_x, int ntiles,
                                                                      VoxAux aux) {
  int tile;
  uint32_t cls, work;
  if (!voxel_tile<SS, true>(f, f, aux, tiles_x, ntiles, tile, cls, work)) return;
  if (COST) {  // as k_voxel_ordered
    const uint32_t w = wave_max_u32(work);
    if ((threadIdx.x & 63) == 0) store_cost(f.tile_cost, tile, tile_bucket(w >> 2), cls, f.cost_diff);
  }
}

// The placing instantiations (sfrt_voxel_render_subset[_aux]), one family over
// SS with AUX as its flag, the planes and the column stride in arguments of their own.  Row-major
// always and outside every tile-order chain: no sorter, no cost record.  Each takes the bound of
// its sibling above (plain: k_voxel_ordered's, planes: k_voxel_aux's).
template <int SS, bool AUX>
__global__ __launch_bounds__(64, AUX ? SFRT_VOX_AUX_WAVES : SFRT_VOX_WAVES) void k_voxel_place(
    VoxFrame f, int tiles_x, int ntiles, VoxAux aux, int xstride) {
  int tile;
  uint32_t cls, work;
  (void)voxel_tile<SS, AUX, true>(f, f, aux, tiles_x, ntiles, tile, cls, work, xstride);
}

// The view batches (sfrt_voxel_render_views[_aux]), one family over SS with AUX as
// its flag on a two-dimensional grid: workgroup (x, y) is tile x, row-major, of view y.  The view's
// record is read from the device table once, at entry, as sphere_trace.hip's view_rec_at reads its
// own: the table is written only by the staging copy that precedes the launch on its stream and
// the address is wave-uniform, so through the constant address space the fields arrive by scalar
// loads, as a band kernel's arrive from its arguments.  They replace the per-camera fields of the
// argument's frame (the camera, dda_qlim, the col / row / dyn tables, the target; the planes for
// AUX); every other field is the argument's, shared by all views.  The tile-order pointers are
// constants here, so the sorter, the order lookup and the cost record fold away.  A wave belongs to
// one view, so raycast()'s fast-DDA vote uses that view's dda_qlim and stays wave-uniform.  Each
// takes the bound of its sibling (plain: k_voxel_ordered's, planes: k_voxel_aux's).
__device__ __forceinline__ VoxViewRec vox_view_rec_at(const VoxViewRec* p, uint32_t view) {
  const __attribute__((address_space(4))) uint32_t* q =
      (const __attribute__((address_space(4))) uint32_t*)(
          (const __attribute__((address_space(4))) char*)p + (size_t)view * sizeof(VoxViewRec));
  uint32_t w[sizeof(VoxViewRec) / 4];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(VoxViewRec) / 4); i++) w[i] = q[i];
  VoxViewRec r;
  __builtin_memcpy(&r, w, sizeof r);
  return r;
}
template <int SS, bool AUX>
__global__ __launch_bounds__(64, AUX ? SFRT_VOX_AUX_WAVES : SFRT_VOX_WAVES) void k_voxel_views(
    VoxFrame f, int tiles_x, int ntiles, const VoxViewRec* views) {
  const VoxViewRec v = vox_view_rec_at(views, blockIdx.y);
  int tile;
  uint32_t cls, work;
  (void)voxel_tile<SS, AUX>(f, v, AUX ? v.aux : VoxAux{}, tiles_x, ntiles, tile, cls, work);
}

// ---- Ray batches: World::Raycast / World::LRaycast for caller-supplied rays
// (sfrt_voxel_cast_rays, sfrt_voxel_cast_shadow_rays) ----
//
// The frame kernels take the fast DDA (reciprocal divisions, plain conversions, the NaN-free axis
// choice) on the host's dda_qlim, which is derived from cam, maxiter and the frame tables' largest
// component.  A caller's rays have neither that origin nor those directions, so a batch wave
// proves the same bound from its own lanes: dda_qlim's argument (sfrt_voxel.cpp) with the lane's
// origin o in cam's place and the lane's own X = max_k |d_k|, m = min_k |d_k| -- one step moves an
// axis by less than S = 2.001 X / m + 0.003 X + 33 while the position is below 2^30, so
// |o|_max + (trips + 1) S <= 2^30 keeps every position of a walk of `trips` steps below 2^30.
// Evaluated in binary32: every term is non-negative (no cancellation) and the seven roundings
// stay within 2^-20 relative, so the sum is held to 2^30 - 2^20 instead; an overflow or a NaN
// compares false.  m >= 2^-60 (recip_ok) is part of it.  DESIGN.md 20 has the argument.
__device__ __forceinline__ bool walk_bounded(V3 o, V3 d, float trips) {
  const float lx = fabsf(d.x), ly = fabsf(d.y), lz = fabsf(d.z);
  const float X = fmaxf(fmaxf(lx, ly), lz), m = fminf(fminf(lx, ly), lz);
  const float P = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
  const float S = 2.001f * (X / m) + 0.003f * X + 33.0f;
  return recip_ok(lx) && recip_ok(ly) && recip_ok(lz) && P + (trips + 1.0f) * S <= 1072693248.0f;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();
}

// One wave per 64 consecutive rays, ray q = 64 * block + lane, through the frame kernels'
// raycast_t.  A lane past the batch's end and a lane with an invalid ray (a non-finite component
// of dir, origin or yscale) get the direction (1, 1, 1), yscale 1 and the origin 0 -- operands
// that vote for the fast DDA -- and stay out of the step loop (BatchRay::live), so they read no
// cell, no billboard and no texel, set no status bit and change no other lane's path: raycast_t's
// other ballots (billboards, the light skip, lraycast) run inside or after the loop, among the
// lanes that marched.  OWN: origins given, no billboards (dnext is NaN, f.dyn is not read);
// without it atan2f(dir.z, dir.x) of VAngleXZ is evaluated per ray, only when there are
// billboards.  SHADE: rgba requested.  Each output is stored under a wave-uniform null test.
// The plain frame kernels' bound, eight waves per SIMD: 63 (camera) / 64 (OWN) VGPRs shaded, 55 / 59
// unshaded, no scratch; under the AUX kernels' seven-wave bound the shaded ones took 66 / 68 and
// measured 4 % slower (tools/kernel_resources.py).
template <bool OWN, bool SHADE>
__global__ __launch_bounds__(64, SFRT_VOX_WAVES) void k_voxel_cast_rays(VoxFrame f, VoxRays a) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * 64 + lane;
  const bool in = q < a.count;
  const long long qc = in ? q : a.count - 1;
  const float* __restrict__ dp = a.dirs + 3 * qc;
  const float rx = dp[0], ry = dp[1], rz = dp[2];
  const float rs = a.yscales ? a.yscales[qc] : 1.0f;
  bool ok = finite3(rx, ry, rz) && fabsf(rs) < __builtin_inff();
  BatchRay ray;
  ray.org = V3{f.cam[0], f.cam[1], f.cam[2]};
  if constexpr (OWN) {
    const float* __restrict__ op = a.origins + 3 * qc;
    ray.org = V3{op[0], op[1], op[2]};
    ok = ok && finite3(ray.org.x, ray.org.y, ray.org.z);
  }
  ray.live = in && ok;
  const V3 dir{ok ? rx : 1.0f, ok ? ry : 1.0f, ok ? rz : 1.0f};
  const float yscale = ok ? rs : 1.0f;
  if (!ok) ray.org = V3{0.0f, 0.0f, 0.0f};
  ray.end = ray.org;
  float atan_dir = 0.0f;
  if constexpr (!OWN) {
    if (f.ndyn > 0) atan_dir = sfrt_math::atan2f(dir.z, dir.x);  // VAngleXZ's ray term (World.cpp:272)
  }
  uint32_t work = 0;
  VoxHit hit;
  uint32_t rgba;
  if (__builtin_amdgcn_ballot_w64(!walk_bounded(ray.org, dir, (float)f.maxiter)))
    rgba = raycast_t<false, false, true, OWN, SHADE>(f, f, dir, yscale, atan_dir, work, hit, ray);
  else
    rgba = raycast_t<true, true, true, OWN, SHADE>(f, f, dir, yscale, atan_dir, work, hit, ray);
  if (in) {  // an invalid ray: face 0, cell -1, steps 0, all-zero bytes elsewhere
    if (a.pos) {
      float* const o = a.pos + 3 * q;
      o[0] = ok ? ray.end.x : 0.0f;
      o[1] = ok ? ray.end.y : 0.0f;
      o[2] = ok ? ray.end.z : 0.0f;
    }
    if (a.depth) a.depth[q] = ok ? hit.depth : 0.0f;
    if (a.cell) a.cell[q] = ok ? hit.cell : -1;
    if (a.face) a.face[q] = ok ? hit.face : 0;
    if (a.steps) a.steps[q] = ok ? hit.steps : 0;
    if constexpr (SHADE) a.rgba[q] = ok ? rgba : 0u;
  }
}

// World::LRaycast for ray q, the same shape, through the shading's lraycast_t.  A lane past the
// end or with an invalid ray (a non-finite component or max_dist, or max_dist past
// kVoxMaxShadowDist) gets origin 0, direction (1, 1, 1) and max_dist 0: it votes for the
// reciprocal divisions and its loop never runs.  The reciprocal divisions only under
// walk_bounded for the ray's own trip limit (lraycast()'s recip_ok alone holds for the shading's
// rays, normalised and from a hit point; a caller's can leave the integers' range, where a
// quotient overflows).  `steps` is lraycast_t's work count.
__global__ __launch_bounds__(64) void k_voxel_shadow_rays(VoxFrame f, VoxShadowRays a) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * 64 + lane;
  const bool in = q < a.count;
  const long long qc = in ? q : a.count - 1;
  const float* __restrict__ op = a.origins + 3 * qc;
  const float* __restrict__ dp = a.dirs + 3 * qc;
  const float ox = op[0], oy = op[1], oz = op[2];
  const float rx = dp[0], ry = dp[1], rz = dp[2];
  const float md = a.max_dists[qc];
  const bool ok = finite3(ox, oy, oz) && finite3(rx, ry, rz) && fabsf(md) < __builtin_inff() &&
                  md <= kVoxMaxShadowDist;
  const V3 org{ok ? ox : 0.0f, ok ? oy : 0.0f, ok ? oz : 0.0f};
  const V3 dir{ok ? rx : 1.0f, ok ? ry : 1.0f, ok ? rz : 1.0f};
  const float max_dist = in && ok ? md : 0.0f;
  const float m2 = max_dist * 2;
  uint32_t work = 0;
  bool free_;
  if (__builtin_amdgcn_ballot_w64(!walk_bounded(org, dir, m2 < 20.0f ? 20.0f : m2)))
    free_ = lraycast_t<false>(f, org, dir, max_dist, work);
  else
    free_ = lraycast_t<true>(f, org, dir, max_dist, work);
  if (in) {
    if (a.free_) a.free_[q] = ok ? (free_ ? 1 : 0) : -1;
    if (a.steps) a.steps[q] = ok ? (int32_t)work : 0;
  }
}

// The grid rewrite of launch_voxel_cells: one 256-lane workgroup per (x, y) row of the box, four
// bytes of the row per lane (a row starts at a 1 KiB boundary, so the full words are aligned
// dword stores).
__global__ __launch_bounds__(256) void k_voxel_cells(uint8_t* __restrict__ cells,
                                                     const uint8_t* __restrict__ codes, int nx, int ny,
                                                     int nz, int by, int bz) {
  const int x = (int)blockIdx.x / by, y = (int)blockIdx.x - x * by;
  const int z0 = 4 * (int)threadIdx.x;
  if (z0 >= bz) return;
  const bool row_in = x < nx && y < ny;
  const uint8_t* src = codes + ((size_t)x * ny + y) * nz;
  uint8_t b[4];
#pragma unroll
  for (int k = 0; k < 4; k++) b[k] = row_in && z0 + k < nz ? src[z0 + k] : (uint8_t)0;
  uint8_t* dst = cells + ((size_t)x << 20) + ((size_t)y << 10) + z0;
  if (z0 + 4 <= bz) {
    *reinterpret_cast<uint32_t*>(dst) =
        (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  } else {
    for (int k = 0; z0 + k < bz; k++) dst[k] = b[k];
  }
}

}  // namespace

long long voxel_tile_key(const VoxFrame& f, long long* tiles) {
  *tiles = 0;
  if (f.sub_w <= 0 || f.sub_rows <= 0) return 0;
  const long long tx = (f.sub_w + 7) / 8, ty = (f.sub_rows + 7) / 8;
  *tiles = tx * ty;
  return (1ll << 62) | ((long long)(f.ss & 3) << 59) | (tx << 28) | ty;
}

namespace {
template <bool COST, int SS>
void launch_voxel_ss(const VoxFrame& f, dim3 grid, long long tiles, void* stream, void* done_event) {
  hipExtLaunchKernelGGL((k_voxel_ordered_ss<COST, SS>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                        (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles);
}
template <bool COST, int SS>
void launch_voxel_aux(const VoxFrame& f, const VoxAux& aux, dim3 grid, long long tiles, void* stream,
                      void* done_event) {
  hipExtLaunchKernelGGL((k_voxel_aux<COST, SS>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                        (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles, aux);
}
template <int SS>
void launch_voxel_place(const VoxFrame& f, const VoxAux* aux, int xstride, dim3 grid, long long tiles,
                        void* stream, void* done_event) {
  if (aux)
    hipExtLaunchKernelGGL((k_voxel_place<SS, true>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                          (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles, *aux, xstride);
  else
    hipExtLaunchKernelGGL((k_voxel_place<SS, false>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                          (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles, VoxAux{}, xstride);
}
}  // namespace

int launch_voxel(const VoxFrame& f, void* stream, void* done_event, const VoxAux* aux,
                 int place_xstride) {
  long long tiles = 0;
  if (voxel_tile_key(f, &tiles) == 0) return 0;
  // the kernel reads the grid through a buffer resource over f.cells (f.cell_bytes) and the tables
  // unguarded: refuse a record whose device pointers were not filled
  if (!f.cells || f.cell_bytes == 0 || !f.col || !f.row || !f.out || !f.status ||
      (f.ndyn > 0 && !f.dyn) || (f.nlights > 0 && !f.lights))
    return -1;
  if (tiles > 0x7ffffffeLL) return -1;
  // row-major unless the host linked this launch into its tile-order chain
  const dim3 grid((unsigned)(tiles + (f.prev_cost ? 1 : 0)));
  if (f.ss < 0 || f.ss > 2) return -1;
  // whole S x S groups: the filter's cross-lane adds rely on it
  if (f.ss && ((f.sub_w | f.sub_row0 | f.sub_rows) & ((1 << f.ss) - 1))) return -1;
  if (aux && !aux->depth && !aux->cell && !aux->face && !aux->steps) return -1;
  if (place_xstride) {  // the placing kernels: row-major, outside every chain
    if (place_xstride < 0 || f.tile_order || f.tile_cost || f.prev_cost) return -1;
    // the last output column's element offset fits the kernels' int
    if ((long long)((f.sub_w - 1) >> f.ss) * place_xstride > 0x7fffffffLL) return -1;
    if (f.ss == 0) launch_voxel_place<0>(f, aux, place_xstride, grid, tiles, stream, done_event);
    else if (f.ss == 1) launch_voxel_place<1>(f, aux, place_xstride, grid, tiles, stream, done_event);
    else launch_voxel_place<2>(f, aux, place_xstride, grid, tiles, stream, done_event);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (aux) {  // the same grid, the plane-writing kernels
    const bool cost = f.tile_cost != nullptr;
    if (f.ss == 0) {
      if (cost) launch_voxel_aux<true, 0>(f, *aux, grid, tiles, stream, done_event);
      else launch_voxel_aux<false, 0>(f, *aux, grid, tiles, stream, done_event);
    } else if (f.ss == 1) {
      if (cost) launch_voxel_aux<true, 1>(f, *aux, grid, tiles, stream, done_event);
      else launch_voxel_aux<false, 1>(f, *aux, grid, tiles, stream, done_event);
    } else {
      if (cost) launch_voxel_aux<true, 2>(f, *aux, grid, tiles, stream, done_event);
      else launch_voxel_aux<false, 2>(f, *aux, grid, tiles, stream, done_event);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  if (f.ss == 1) {
    if (f.tile_cost) launch_voxel_ss<true, 1>(f, grid, tiles, stream, done_event);
    else launch_voxel_ss<false, 1>(f, grid, tiles, stream, done_event);
  } else if (f.ss == 2) {
    if (f.tile_cost) launch_voxel_ss<true, 2>(f, grid, tiles, stream, done_event);
    else launch_voxel_ss<false, 2>(f, grid, tiles, stream, done_event);
  } else if (f.tile_cost)
    hipExtLaunchKernelGGL(k_voxel_ordered<true>, grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                          (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles);
  else
    hipExtLaunchKernelGGL(k_voxel_ordered<false>, grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                          (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace {
template <int SS>
void launch_views(const VoxFrame& f, const VoxViewRec* views, bool aux, dim3 grid, long long tiles,
                  void* stream, void* done_event) {
  if (aux)
    hipExtLaunchKernelGGL((k_voxel_views<SS, true>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                          (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles, views);
  else
    hipExtLaunchKernelGGL((k_voxel_views<SS, false>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                          (hipEvent_t)done_event, 0, f, (int)((f.sub_w + 7) / 8), (int)tiles, views);
}
}  // namespace

bool voxel_views_grid_ok(const VoxFrame& f, int count) {
  long long tiles = 0;
  if (voxel_tile_key(f, &tiles) == 0) return false;
  // work-items per grid dimension are 32 bits, workgroups in all at most 2^31 - 1
  return count > 0 && tiles * 64 <= 0xffffffffLL && tiles * count <= 0x7fffffffLL;
}

int launch_voxel_views(const VoxFrame& f, const VoxViewRec* dev_views, int count, bool aux,
                       void* stream, void* done_event) {
  if (!voxel_views_grid_ok(f, count) || count > 65535 || !dev_views) return -1;
  long long tiles = 0;
  (void)voxel_tile_key(f, &tiles);
  // as launch_voxel: the grid through a buffer resource; the per-view tables come from the records
  if (!f.cells || f.cell_bytes == 0 || !f.status || (f.nlights > 0 && !f.lights)) return -1;
  if (f.tile_order || f.tile_cost || f.prev_cost || f.next_order) return -1;
  if (f.ss < 0 || f.ss > 2 || f.sub_row0 != 0) return -1;
  if (f.ss && ((f.sub_w | f.sub_rows) & ((1 << f.ss) - 1))) return -1;
  const dim3 grid((unsigned)tiles, (unsigned)count);
  if (f.ss == 0) launch_views<0>(f, dev_views, aux, grid, tiles, stream, done_event);
  else if (f.ss == 1) launch_views<1>(f, dev_views, aux, grid, tiles, stream, done_event);
  else launch_views<2>(f, dev_views, aux, grid, tiles, stream, done_event);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace {
template <bool OWN, bool SHADE>
void launch_rays(const VoxFrame& f, const VoxRays& a, dim3 grid, void* stream, void* done_event) {
  hipExtLaunchKernelGGL((k_voxel_cast_rays<OWN, SHADE>), grid, dim3(64), 0, (hipStream_t)stream, nullptr,
                        (hipEvent_t)done_event, 0, f, a);
}
}  // namespace

int launch_voxel_rays(const VoxFrame& f, const VoxRays& a, void* stream, void* done_event) {
  if (a.count == 0) return 0;
  // as launch_voxel: the grid through a buffer resource, the tables unguarded
  if (!f.cells || f.cell_bytes == 0 || !f.status || (f.ndyn > 0 && !f.dyn) || (f.nlights > 0 && !f.lights))
    return -1;
  if (!a.dirs || a.count < 0 || a.count > 0x7fffffffLL) return -1;
  if (!a.pos && !a.depth && !a.cell && !a.face && !a.steps && !a.rgba) return -1;
  const dim3 grid((unsigned)((a.count + 63) / 64));
  if (a.origins) {
    if (a.rgba) launch_rays<true, true>(f, a, grid, stream, done_event);
    else launch_rays<true, false>(f, a, grid, stream, done_event);
  } else {
    if (a.rgba) launch_rays<false, true>(f, a, grid, stream, done_event);
    else launch_rays<false, false>(f, a, grid, stream, done_event);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_voxel_shadow_rays(const VoxFrame& f, const VoxShadowRays& a, void* stream, void* done_event) {
  if (a.count == 0) return 0;
  if (!f.cells || f.cell_bytes == 0) return -1;
  if (!a.origins || !a.dirs || !a.max_dists || a.count < 0 || a.count > 0x7fffffffLL) return -1;
  if (!a.free_ && !a.steps) return -1;
  hipExtLaunchKernelGGL(k_voxel_shadow_rays, dim3((unsigned)((a.count + 63) / 64)), dim3(64), 0,
                        (hipStream_t)stream, nullptr, (hipEvent_t)done_event, 0, f, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_voxel_cells(uint8_t* cells, const uint8_t* codes, int nx, int ny, int nz, int bx, int by,
                       int bz, void* stream) {
  // the box must hold the world and stay inside the key space (kVoxMax*), the rows inside 1 KiB
  if (!cells || (nx > 0 && !codes) || nx < 0 || ny < 0 || nz < 0 || bx < nx || by < ny || bz < nz ||
      bx > kVoxMaxX || by > kVoxMaxY || bz > kVoxMaxZ)
    return -1;
  if (bx == 0 || by == 0 || bz == 0) return 0;
  hipLaunchKernelGGL(k_voxel_cells, dim3((unsigned)((long long)bx * by)), dim3(256), 0,
                     (hipStream_t)stream, cells, codes, nx, ny, nz, by, bz);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sfrt
