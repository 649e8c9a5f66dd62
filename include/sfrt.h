/*
 * sfrt.h -- C ABI of the MI355X sphere-cave tracer (libsfrt.so).
 *
 * Drop-in for the reference's CPU frame fill
 *   void SphereWorld::UpdateImage(sf::Image* v, short ystart, short yadd,
 *                                 short xstart, short xadd)
 *   (/root/reference/Raytracing/SphereWorld.h:43, SphereWorld.cpp:83-112)
 * and the scene state it reads (SphereWorld.h:50-57,74).  `sf::Uint8` is
 * `unsigned char`, so an SFML caller passes its own RGBA8 buffer (the bytes
 * it would give to sf::Texture::update / sf::Image::create); see
 * INTEGRATION.md.  Plain C types only: no HIP, torch or SFML types cross this
 * boundary.  All functions return 0 (SFRT_OK) or a negative SFRT_E_* code.
 * A world is safe to call from several host threads (calls serialise on an
 * internal mutex); distinct worlds are independent.
 */
#ifndef SFRT_H
#define SFRT_H

#include <stdint.h>

#if defined(__GNUC__)
#define SFRT_API __attribute__((visibility("default")))
#else
#define SFRT_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SFRT_OK 0
#define SFRT_E_INVALID -1      /* bad argument (null, size <= 0, non-finite value, radius <= 0) */
#define SFRT_E_EMPTY -2        /* no spheres: the reference throws std::out_of_range (SphereWorld.cpp:373) */
#define SFRT_E_NO_TEXTURE -3   /* textures[0] not loaded (SphereWorld.cpp:52) */
#define SFRT_E_TOO_MANY -4     /* more than SFRT_MAX_SPHERES spheres */
#define SFRT_E_HIP -5          /* HIP runtime error (no device, launch or copy failure) */
#define SFRT_E_MARCH_LIMIT -6  /* a ray exceeded SFRT_MAX_ITERATIONS march steps */
#define SFRT_E_TEXEL -7        /* a texel index fell outside the texture (reference: out-of-bounds read) */

#define SFRT_MAX_SPHERES 1024
#define SFRT_MAX_ITERATIONS (1 << 20)
#define SFRT_TEXTURE_SLOTS 10  /* sf::Image* textures = new sf::Image[10] (SphereWorld.h:74) */

/* sf::Vector3f pos + float radius of struct Sphere (SphereWorld.h:23-29). */
typedef struct {
  float x, y, z, radius;
} sfrt_sphere;

/* The fields of struct Camera (SphereWorld.h:10-21) that the frame fill reads.
 * fov_h / fov_v are in radians, i.e. after `cam.fovH *= PI / 180.0f`
 * (SphereWorld.cpp:72-73); sfrt_deg_to_rad reproduces that conversion. */
typedef struct {
  float pos[3];
  float rotation;
  float hrotation;
  float fov_h;
  float fov_v;
} sfrt_camera;

/* Float intermediates of one pixel (parity/debug): final march position,
 * drawSphere, march iterations, xcoord/ycoord/brightness of
 * SphereWorld.cpp:373-375, texel coordinates and the RGBA8 result. */
typedef struct {
  float pos[3];
  int32_t draw;
  int32_t iters;
  float xcoord, ycoord, brightness;
  uint32_t texel[2];
  uint32_t rgba;
} sfrt_pixel_dump;

typedef struct sfrt_world sfrt_world;

/* ---- world lifetime (SphereWorld::SphereWorld / ~SphereWorld, SphereWorld.cpp:43-81) ----
 * A new world has width 320, height 180, camera at the origin with
 * fov 75/47 degrees converted to radians, no spheres and no textures. */
SFRT_API int sfrt_world_create(int hip_device, sfrt_world** out);
SFRT_API void sfrt_world_destroy(sfrt_world* w);

/* ---- scene state ---- */
SFRT_API int sfrt_world_set_size(sfrt_world* w, int width, int height);          /* SphereWorld::width/height */
SFRT_API int sfrt_world_get_size(const sfrt_world* w, int* width, int* height);
SFRT_API int sfrt_world_set_camera(sfrt_world* w, const sfrt_camera* cam);       /* SphereWorld::cam */
SFRT_API int sfrt_world_get_camera(const sfrt_world* w, sfrt_camera* cam);
/* textures[slot].loadFromFile(...) (SphereWorld.cpp:52): RGBA8 rows, w*h*4 bytes. Slot 0 is sampled.
   Stream-ordered, no device-wide wait: frames queued before the call read the old texels, frames
   queued after it (on any stream) the new ones. */
SFRT_API int sfrt_world_load_texture(sfrt_world* w, int slot, const uint8_t* rgba, int tex_w, int tex_h);
/* AddSphere (SphereWorld.cpp:177-190): append, drop contained spheres, re-sort. */
SFRT_API int sfrt_world_add_sphere(sfrt_world* w, float x, float y, float z, float radius);
/* Replace the sphere list verbatim (caller order = the order the march visits). */
SFRT_API int sfrt_world_set_spheres(sfrt_world* w, const sfrt_sphere* spheres, int count);
SFRT_API int sfrt_world_get_spheres(const sfrt_world* w, sfrt_sphere* out, int capacity, int* count);
/* Extension ("all textures"): a texture slot per sphere, in the
 * current sphere order (count == number of spheres); slots travel with their spheres
 * through AddSphere / UpdateSpheres.  Default 0 = textures[0] everywhere = the
 * reference (SphereWorld.cpp:376-377 samples textures[0] only). */
SFRT_API int sfrt_world_set_sphere_textures(sfrt_world* w, const int32_t* slots, int count);
SFRT_API int sfrt_world_get_sphere_textures(sfrt_world* w, int32_t* out, int capacity, int* count);
/* UpdateSpheres sort part (SphereWorld.cpp:199-212): stable by |c - cam.pos| + r. */
SFRT_API int sfrt_world_update_spheres(sfrt_world* w);

/* ---- the frame fill ----
 * SphereWorld::UpdateImage(v, ystart, yadd, xstart, xadd): renders pixels
 * {i = xstart + k*xadd < width} x {j = ystart + l*yadd < height} into the
 * caller's host buffer `pixels` (width*height*4 bytes, RGBA8 row-major,
 * pitch 4*width) and writes no other byte.  Returns when the bytes are in
 * `pixels`. */
SFRT_API int sfrt_world_update_image(sfrt_world* w, uint8_t* pixels, int ystart, int yadd, int xstart,
                            int xadd);

/* Device-resident frame fill for the display / multi-GPU path: rows
 * [row0, row0 + rows) of the width x height frame into `dev_pixels` (device
 * memory on this world's device; row r of the band at dev_pixels +
 * (r - row0) * pitch_bytes).  Rays use the GLOBAL row index, so row bands
 * rendered on different GPUs tile the single-GPU frame byte for byte.
 * Asynchronous on `hip_stream` (a hipStream_t; NULL = the HIP null stream);
 * call sfrt_world_check(w, hip_stream) to synchronise and read the
 * march-limit / texel status of the launches since the last check. */
SFRT_API int sfrt_world_render_band(sfrt_world* w, void* dev_pixels, int64_t pitch_bytes, int row0,
                           int rows, void* hip_stream);
SFRT_API int sfrt_world_check(sfrt_world* w, void* hip_stream);

/* ---- the frame fill's per-pixel planes: depth, sphere index, march steps ----
 * For pixel (i, j) of the world's width x height frame there are three optional planes of
 * 4 bytes per pixel, written by the same launch that writes the colour:
 *   depth  (float):   the binary32 value of VLength(r->pos - cam.pos) as SphereWorld.cpp:375
 *                     evaluates it -- the operand of std::max(.., 3.0f), not the clamped
 *                     value: sqrtf((ex*ex + ey*ey) + ez*ez) with e = pos - cam per component,
 *                     correctly rounded, no contraction.  (The colour's brightness is 1 for
 *                     every depth below 3 and carries no depth there; this plane does.)
 *   sphere (int32_t): drawSphere after the march (SphereWorld.cpp:360-369), an index into the
 *                     world's current sphere order, the order sfrt_world_get_spheres returns.
 *   steps  (int32_t): the loop trips of SphereWorld.cpp:362, the first one included: the same
 *                     count as sfrt_pixel_dump.iters.
 * With SFRT_OPT_SUPERSAMPLE S = 2 or 4 the colour is the box-filtered pixel as always, and the
 * three planes describe the output pixel's FIRST SAMPLE, sample pixel (S*i, S*j) of the
 * S*width x S*height frame: point-sampled, as a resolved depth buffer takes sample 0; no
 * filtered, minimum or per-sample depth.
 * The planes do not depend on the texel: a frame whose status is SFRT_E_TEXEL still has defined
 * planes.  Pixels of a ray that hit the march guard (SFRT_E_MARCH_LIMIT) are unspecified, as
 * their colour is.
 * Planes must not overlap each other or the colour target; that is the caller's duty.
 * Both calls below return SFRT_E_INVALID, with nothing queued or written, when all three
 * planes are NULL, or (render_band_aux) a non-NULL plane's pitch is not a multiple of 4 or is
 * below 4*width; a NULL plane's pitch is ignored.  The plain calls' own argument checks apply
 * unchanged, and the plain calls keep their behaviour exactly.
 * The planes come from kernels of their own, which compute their ray directions: an aux call
 * neither reads, fills nor invalidates the ray cache (SFRT_OPT_RAY_CACHE_MB) and leaves the
 * counters of sfrt_world_ray_cache_stats alone.  sfrt_world_submit_frame and sfrt_multi_* have no
 * planes; the voxel renderer has its own (sfrt_voxel_render_band_aux), and the GLSL renderer
 * reuses this record (sfrt_glsl_draw_aux). */
typedef struct {
  void* depth;  int64_t depth_pitch_bytes;   /* float   per pixel, or NULL */
  void* sphere; int64_t sphere_pitch_bytes;  /* int32_t per pixel, or NULL */
  void* steps;  int64_t steps_pitch_bytes;   /* int32_t per pixel, or NULL */
} sfrt_aux_planes;
/* sfrt_world_render_band plus the planes (device memory on this world's device): same rows,
 * same global row index, same stream semantics, same status word, same place in the adaptive
 * tile order (sfrt_world_row_costs works after it); row r of a plane at
 * plane + (r - row0) * its pitch. */
SFRT_API int sfrt_world_render_band_aux(sfrt_world* w, void* dev_pixels, int64_t pitch_bytes,
                                        const sfrt_aux_planes* aux, int row0, int rows,
                                        void* hip_stream);
/* sfrt_world_update_image plus host planes of width*height elements (pitch 4*width); any of
 * depth / sphere / steps may be NULL (not all); only addressed pixels are written, in every
 * plane.  On SFRT_E_TEXEL the planes are written and `pixels` is left as
 * sfrt_world_update_image leaves it on that status (unwritten). */
SFRT_API int sfrt_world_update_image_aux(sfrt_world* w, uint8_t* pixels, float* depth,
                                         int32_t* sphere, int32_t* steps, int ystart, int yadd,
                                         int xstart, int xadd);

/* ---- UpdateImage's pixel subsets in place in a device-resident frame ----
 * sfrt_world_update_image for a frame that stays on the GPU between calls, as the reference's
 * gameImage stays alive between its RenderThreads' UpdateImage(&gameImage, num, 8, cycle, 4)
 * calls.  `dev_frame` is the WHOLE width x height frame in device memory on this world's device,
 * row j at dev_frame + j * pitch_bytes.  The call writes the 4 bytes of every pixel
 * {i = xstart + k*xadd < width} x {j = ystart + l*yadd < height} -- the bytes
 * sfrt_world_update_image writes for the same arguments and state -- and no other byte: not the
 * unaddressed pixels, not the padding past 4*width of a row.  The aux call writes the same
 * elements of every non-NULL plane (whole-frame planes, each with its own pitch; the values of
 * sfrt_world_update_image_aux) and nothing of a NULL one.
 * Asynchronous on `hip_stream` with sfrt_world_render_band's stream semantics (NULL = the null
 * stream, ordered behind the last texture upload, status through sfrt_world_check).
 * SFRT_OPT_SUPERSAMPLE, SFRT_OPT_CULL and SFRT_OPT_RAYS_PER_LANE are honoured as
 * sfrt_world_update_image honours them.  The launch is row-major and stands outside the
 * adaptive tile order and the ray cache: it leaves sfrt_world_row_costs and
 * sfrt_world_ray_cache_stats as they were.
 * SFRT_E_INVALID, with nothing queued or written: a NULL world or frame, ystart < 0, xstart < 0,
 * yadd <= 0, xadd <= 0, pitch_bytes not a multiple of 4 or below 4*width, and for the aux call
 * render_band_aux's plane rules.  The arguments that need no world are checked first, then the
 * world's own validation (SFRT_E_EMPTY, SFRT_E_NO_TEXTURE, ...: as for render_band), then the
 * pitches against the world's width -- the same order in both worlds.  An
 * empty subset (xstart >= width or ystart >= height) returns SFRT_OK with nothing queued. */
SFRT_API int sfrt_world_render_subset(sfrt_world* w, void* dev_frame, int64_t pitch_bytes,
                                      int ystart, int yadd, int xstart, int xadd, void* hip_stream);
SFRT_API int sfrt_world_render_subset_aux(sfrt_world* w, void* dev_frame, int64_t pitch_bytes,
                                          const sfrt_aux_planes* aux, int ystart, int yadd,
                                          int xstart, int xadd, void* hip_stream);

/* ---- a batch of camera views of the world in one launch ----
 * The other eye of a stereo pair, the six faces of a probe's cube map, a split screen, a mini-map,
 * many small agent or thumbnail views: each a whole width x height frame of this world from a
 * camera of its own, into a target of its own, all in one kernel launch.
 * Definition: with the world as it stands at the call, view k receives exactly the bytes that
 *   sfrt_world_set_camera(w, &views[k].cam);
 *   sfrt_world_update_spheres(w);                 -- with SFRT_VIEWS_SORT only
 *   sfrt_world_render_band(w, views[k].dev_pixels, pitch_bytes, 0, height, s);
 * would write on a copy of that world (the aux call: sfrt_world_render_band_aux with planes[k]),
 * and the call writes no other byte.  Every view sorts from the world's current sphere order, not
 * from view k-1's, and the per-sphere texture slots travel with their spheres; the sphere plane
 * of a sorted view indexes that view's sorted order.  Whole frames only.
 * The world itself is left as it was: its camera, its sphere list and order, the sphere
 * textures, the tile-order chains, the ray cache and tile records (sfrt_world_ray_cache_stats)
 * and the last fill (sfrt_world_row_costs).
 * Asynchronous on `hip_stream` with sfrt_world_render_band's stream semantics; the march-limit
 * and texel bits of every view go into the world's status word (sfrt_world_check).
 * SFRT_OPT_SUPERSAMPLE, SFRT_OPT_CULL and SFRT_OPT_RAYS_PER_LANE are honoured (0 rays per lane:
 * the row-major kernel table's choice, as sfrt_world_render_subset); the launch is row-major within
 * a view and view-major across views, so SFRT_OPT_TILE_ORDER and SFRT_OPT_RAY_CACHE_MB have no
 * influence.
 * count == 0 returns SFRT_OK with nothing queued.  SFRT_E_INVALID, with nothing queued or written:
 * a NULL world or `views`, count < 0 or > SFRT_MAX_VIEWS, unknown flag bits, pitch_bytes not a
 * multiple of 4 or below 4*width, a NULL or not 4-byte-aligned dev_pixels or a camera
 * sfrt_world_set_camera would refuse in any view, (aux) NULL `planes`, an entry with all three
 * planes NULL or with a pitch sfrt_world_render_band_aux would refuse, or a grid the device cannot
 * be given in one launch (more than 2^31 - 1 tiles over all views, or more than 2^26 - 1 tiles in
 * one).  The world's own validation (SFRT_E_EMPTY, SFRT_E_NO_TEXTURE, SFRT_E_TOO_MANY) applies
 * unchanged.  Targets (and planes) that overlap are the caller's responsibility. */
#define SFRT_MAX_VIEWS 1024
#define SFRT_VIEWS_SORT 1          /* flags bit 0: UpdateSpheres' sort per view */
typedef struct {
  sfrt_camera cam;                 /* this view's SphereWorld::cam (voxel: World::cam) */
  void* dev_pixels;                /* its width x height RGBA8 target, rows pitch_bytes apart */
} sfrt_view;
SFRT_API int sfrt_world_render_views(sfrt_world* w, const sfrt_view* views, int count,
                                     int64_t pitch_bytes, int flags, void* hip_stream);
SFRT_API int sfrt_world_render_views_aux(sfrt_world* w, const sfrt_view* views,
                                         const sfrt_aux_planes* planes /* count entries */,
                                         int count, int64_t pitch_bytes, int flags, void* hip_stream);

/* Estimated work per pixel row of the world's last frame fill that ran in the adaptive
 * tile order (sfrt_world_render_band, sfrt_world_submit_frame; SFRT_OPT_TILE_ORDER on):
 * *row0, *rows = the global rows it covered, costs[i] (i < *rows <= capacity) = the
 * ray-steps of row *row0 + i, from the per-tile march-step classes that launch recorded
 * (each pixel costs its tile's class steps plus ~4 for shading).  For cost-weighted row
 * bands (sfrt_multi_cost_bands).  Synchronises with that fill; SFRT_E_INVALID if no
 * such fill exists (or capacity is short). */
SFRT_API int sfrt_world_row_costs(sfrt_world* w, float* costs, int capacity, int* row0, int* rows);

/* Pipelined frame fill for the display path: renders the
 * whole width x height frame of the world's current state into `pixels`
 * (width*height*4 bytes) without blocking, then copies it back while the
 * caller submits the next frame (two frames in flight).  `pixels` should come
 * from sfrt_host_alloc (pinned: the copy overlaps compute and runs at PCIe
 * rate); it must stay valid until sfrt_world_wait_frame(ticket) returns, and
 * then holds the same bytes sfrt_world_update_image(w, pixels, 0, 1, 0, 1)
 * would have written.  The scene/camera are snapshotted at submit time. */
SFRT_API int sfrt_world_submit_frame(sfrt_world* w, uint8_t* pixels, int64_t* ticket);
SFRT_API int sfrt_world_wait_frame(sfrt_world* w, int64_t ticket);
SFRT_API int sfrt_host_alloc(void** ptr, int64_t bytes);
/* hipHostFree underneath: it returns only once the whole device is idle (profiles/r6u_hip_alloc_calls.txt),
   so free pinned frames at shutdown or between bursts, not between frames. */
SFRT_API int sfrt_host_free(void* ptr);

/* Float intermediates for `count` pixels (ij = i0, j0, i1, j1, ...), synchronous: the
 * march position, drawSphere and loop trips of SphereWorld.cpp:362-372, xcoord, ycoord,
 * brightness and the texel of :373-377, and the RGBA8 pixel, read out of the frame-fill
 * kernel itself (its DUMP instantiation renders the whole frame with the world's options:
 * tile shape, culling, and -- SFRT_OPT_TILE_ORDER on -- three launches in the adaptive
 * order).  A pixel may be listed more than once. */
SFRT_API int sfrt_world_trace_points(sfrt_world* w, const int32_t* ij, int count, sfrt_pixel_dump* out);

/* ---- batched ray queries: SphereWorld::Raycast (SphereWorld.cpp:355-382) for caller-supplied rays ----
 * A valid ray.  `dirs` holds 3 floats per ray, un-normalised, exactly as Raycast receives
 * r->dir.  `origins` holds 3 floats per ray.  origins == NULL means every ray starts at the
 * world's cam.pos, as in the reference; the position is snapshotted at the call.
 * Ray q is Raycast with cam.pos replaced by its origin o, in three places:
 *   - pos = o.
 *   - dir = d / sqrtf((dx*dx + dy*dy) + dz*dz) per component.
 *   - Lines :359-372 run as written, including the first trip from pos == o.
 *   - The tail :373-381 uses brightness = 3 / max(VLength(pos - o), 3) and the sphere's texture
 *     slot (sfrt_world_set_sphere_textures is honoured).
 * Arithmetic is binary32, round to nearest, no contraction, with correctly rounded / and sqrt.
 * The transcendentals are sfrt_math's, as everywhere else.
 * An invalid ray.  A ray is invalid when any direction or origin component is not finite, or
 * when s = (dx*dx + dy*dy) + dz*dz is not a finite normal number.  That covers zero, underflow
 * and overflow.  It is decided per ray before the march.  It is never marched.  It gets
 * sphere = -1, and every other requested output is all-zero bytes.  It must not change any
 * other ray's result.  It sets no status bit.
 * Return codes and edge cases.  count == 0 returns SFRT_OK and writes nothing.
 * SFRT_E_INVALID, with nothing queued or written, for: a NULL world; NULL dirs; count < 0 or
 * count > 2^31-1; all five outputs NULL; a non-NULL pointer that is not 4-byte aligned.
 * SFRT_E_EMPTY when there are no spheres.  SFRT_E_NO_TEXTURE only when rgba is requested: a
 * world without textures can still answer pos, depth, sphere and steps.  Overlapping buffers
 * are the caller's responsibility.
 * Status.  The status bits are the frame fill's own: march guard, and texel outside the texture
 * (only when rgba is requested).  The device call leaves them to sfrt_world_check(w,
 * hip_stream).  The host call returns the code; on SFRT_E_TEXEL it writes every output except
 * rgba, as sfrt_world_update_image_aux does.
 * Options and shared state.  SFRT_OPT_CULL is honoured; the bytes are the same either way.
 * SFRT_OPT_SUPERSAMPLE, SFRT_OPT_RAYS_PER_LANE and SFRT_OPT_TILE_ORDER are ignored.  The call
 * joins no tile-order chain.  It neither reads, fills nor invalidates the ray cache or the tile
 * records.  It leaves sfrt_world_ray_cache_stats, sfrt_world_tile_record_bytes and
 * sfrt_world_row_costs exactly as they were.
 * Concurrency.  Calls serialise on the world's mutex; the scene, camera and options are
 * snapshotted at the call, as for sfrt_world_render_band. */
typedef struct {          /* every member: one element per ray, or NULL; not all NULL */
  float*    pos;          /* 3 floats per ray, packed x,y,z (12 B per ray): r->pos after the march */
  float*    depth;        /* VLength(r->pos - origin) as :375 evaluates it, before std::max(.., 3.0f) */
  int32_t*  sphere;       /* drawSphere (:360-369), index into the current sphere order; -1: invalid ray */
  int32_t*  steps;        /* loop trips of :362, the first one included; 0: invalid ray */
  uint8_t*  rgba;         /* 4 bytes per ray: r->c of :373-381 */
} sfrt_ray_hits;

/* device memory on the world's device, asynchronous on hip_stream; status via sfrt_world_check */
SFRT_API int sfrt_world_cast_rays_device(sfrt_world* w, const float* dev_dirs, const float* dev_origins,
                                         int64_t count, const sfrt_ray_hits* dev_out, void* hip_stream);
/* host memory, synchronous */
SFRT_API int sfrt_world_cast_rays(sfrt_world* w, const float* dirs, const float* origins,
                                  int64_t count, const sfrt_ray_hits* out);

/* Options: SFRT_OPT_CULL (1 = per-wave sphere culling, default; 0 = visit
 * every sphere -- same bytes, slower; used by A/B parity tests).
 * SFRT_OPT_RAYS_PER_LANE (0 = default): pixels per lane R of the frame-fill
 * kernel, i.e. its (8R)x8 tile width; 1-4 force that shape (parity tests run
 * every shipped tile shape; same bytes), 0 lets the kernel table choose
 * (sphere_trace.hip trace_rays).
 * SFRT_OPT_TILE_ORDER (1 = default): sfrt_world_render_band dispatches the tiles
 * of a frame longest-first by the march steps an earlier render_band of the same
 * geometry recorded (two frames back; the sort runs inside the next launch);
 * 0 = row-major order.  Scheduling only: same bytes either way.
 * SFRT_OPT_SUPERSAMPLE (1 = default, today's frame byte for byte; 2 or 4; any other value
 * returns SFRT_E_INVALID and changes nothing): S x S samples per pixel, box-filtered inside
 * the frame-fill kernel.  The samples of output pixel (i, j) of the width x height frame are
 * the pixels (S*i + k, S*j + l), 0 <= k, l < S, of the reference's frame fill at width
 * S*width and height S*height (SphereWorld.cpp:85-106 evaluated with those sizes, so
 * hIncreaseBy = cam.fovH / (S*width) * 2), each marched and shaded to RGBA8 as always (the
 * texel rule and both status bits per sample); each of the four output bytes, alpha
 * included, is (sum of the S*S sample bytes + S*S/2) >> log2(S*S), the round-half-up mean.
 * Honoured by sfrt_world_update_image (its strides address output pixels; only those are
 * written), sfrt_world_render_band (global output rows; bands tile the frame byte for
 * byte) and sfrt_world_submit_frame: sizes, pitches, rows and buffers stay in output pixels,
 * and only output pixels are stored and copied.  A frame call returns SFRT_E_INVALID when
 * S*width, S*height or their tile grid exceed what one launch can take.
 * sfrt_world_trace_points ignores the option: it dumps the 1x pixel.
 * sfrt_world_row_costs returns one cost per output row (the sum over its S sample rows,
 * constant over groups of 8 / S rows), and only for a fill made at the current factor.
 * Averaged alphas are no longer 0 or 255: see sfrt_world_alpha_binary.
 * SFRT_OPT_RAY_CACHE_MB (512 = default; 0 = off; negative values return SFRT_E_INVALID): the
 * device memory, in MiB per world, that the world may spend on caching primary ray directions.
 * The direction of a pixel's ray does not depend on the camera position, the spheres or the
 * textures, only on the view rotation, the fields of view, the frame, band and subset
 * geometry, the supersampling factor and the tile shape.  When a stream's second consecutive
 * sfrt_world_render_band / sfrt_world_submit_frame keeps all of those, the directions are
 * written once (12 bytes per ray, 95 MiB for a 4K frame) and later launches load them and
 * skip the ray setup; any launch that changes one of them renders as without the cache, so a
 * camera that turns every frame never fills.  Same bytes either way.  A cache that would
 * take the world past the limit is not created; lowering the limit below what is held waits
 * for the device and frees every cache.  See sfrt_world_ray_cache_stats.
 * The option also governs the tile records that ride with the directions: one 32-byte record
 * per tile (the tile's culling cone and grid position, which depend on the same things),
 * written by the same fill, read by the same launches and freed with the directions.  They
 * are not counted against the limit (0.3 % of the directions' size at 4K); 0 turns both off.
 * See sfrt_world_tile_record_bytes.
 * It governs the cull cache as well.  What a tile's wave culls before it marches -- which
 * spheres can pass for some ray of the tile, and between which along-ray distances -- depends
 * on the tile's cone, the camera position, the sphere count and each sphere's centre and
 * radius, not on the textures or the spheres' texture slots.  When a stream's second consecutive
 * launch keeps all of those (a camera at rest in a scene at rest) and reads the ray cache, the
 * result is written once (528 bytes per tile, 16 MiB for a 4K frame; 784 above 64 spheres) and
 * later launches load it; any launch that changes one of them -- the library compares the values,
 * sphere by sphere -- culls for itself as before, so a walking camera or a sphere that moves
 * every frame never fills.  Same bytes either way.  These bytes count against the limit: a cull
 * cache that would take the world past it is not created.  See sfrt_world_cull_cache_stats.
 * SFRT_OPT_HIT_CACHE_MB (512 = default; 0 = off; negative values return SFRT_E_INVALID): the
 * device memory, in megabytes of 10^6 bytes per world (not MiB: the default then holds two
 * streams' 4K frames, 2 x 132.7 MB, and leaves an 8K frame's 530.8 MB out, which would fit 512
 * MiB), that the world may spend on the hit cache -- a budget of its own, beside
 * SFRT_OPT_RAY_CACHE_MB's and not counted against it.  Where a ray's march ends and
 * on which sphere depends on exactly what the cull cache depends on -- the ray's direction, the
 * camera position, the sphere count and each sphere's centre and radius -- and not on the
 * textures or the spheres' texture slots.  While a stream's launches read the cull cache, the
 * second consecutive launch of one such state also writes each ray's march result (16 bytes per
 * ray: 132.7 MB for a 4K frame, per stream that renders such frames; supersampled, per sample),
 * and later launches of that state do not march at all: they shade from the stored results with
 * the current textures and texture slots, the same bytes as a marching launch and the same
 * status (a texel outside its texture included).  Any launch that changes the state renders as
 * without the hit cache, so a walking or turning camera or a moving sphere never fills.  The hit
 * cache lives on the cull cache: SFRT_OPT_RAY_CACHE_MB 0 turns it off with the rest, and whatever
 * refills the directions or the cull cache drops it.  A hit cache that would take the world past
 * the limit is not created (at the default an 8K frame's 530.8 MB: raise the option to 600 to
 * serve such frames from it) and the launch stays on the cull cache; lowering the limit below what is held waits
 * for the device and frees every hit cache.  sfrt_world_row_costs keeps answering from the last
 * launch that marched.  See sfrt_world_hit_cache_stats.
 * SFRT_OPT_TEXEL_CACHE (1 = default; 0 = off; negative values return SFRT_E_INVALID): the texel
 * cache on top of the hit cache.  What a launch that shades from the hit cache still computes per
 * ray -- the texel's index in the texture atlas -- depends on the hit cache's state and on the
 * texture sizes and the spheres' texture slots, not on the textures' contents.  While those stand
 * still too, the second consecutive launch that reads the hit cache also writes, per ray, that
 * index and the brightness (8 bytes per ray: 66.4 MB for a 4K frame; supersampled, per sample),
 * and later launches read those 8 bytes in place of the 16 of the hit cache and no sphere record:
 * the same bytes and the same status.  Loading a texture of the same size into a slot keeps the
 * cache (the texels are read every frame); a texture of another size, another slot for a sphere,
 * or a load that moves another slot in the atlas makes the next launch shade from the hit cache,
 * which stays allocated, and the one after write the indices again.  The bytes count against
 * SFRT_OPT_HIT_CACHE_MB beside the hit cache's (two 4K streams: 2 x (132.7 + 66.4) = 398 MB);
 * where they do not fit, launches stay on the hit cache.  Whatever drops or refills the hit cache
 * drops the texel cache; setting the option to 0 waits for the device and frees the texel caches
 * only.  See sfrt_world_texel_cache_stats.
 * SFRT_OPT_COMPACT_TEXELS (1 = default; 0 = off; 2 = every eligible launch; other values return
 * SFRT_E_INVALID): the compact layer on top of the texel cache.  At 1 it serves the launches it was
 * measured to pay for by the project's rule -- four pixels per lane (frames of about 4K and more)
 * with at most 64 spheres -- and at 2 also the others (smaller frames, more spheres: a gain of 4 to
 * 11 % that the rule did not confirm).  A pixel's bytes depend on the brightness only through
 * the 256 products with a channel byte, so the brightness can be replaced by one of 20,229 classes
 * (15 bits) without changing a byte; while no sphere's texture ends beyond texel 65,535 of the
 * atlas and the world is not supersampled, the second consecutive launch that reads the texel
 * cache also writes each ray as 4 bytes (33.2 MB for a 4K frame) and later launches read those in
 * place of the 8: the same bytes and the same status.  The bytes count against
 * SFRT_OPT_HIT_CACHE_MB after the hit and texel caches have theirs; where they do not fit, or the
 * atlas is larger, launches stay on the texel cache, which stays allocated either way.  Whatever
 * drops or refills the texel cache of a stream drops its compact layer first, so within a stream
 * the layer never keeps a lower one from filling; between streams its bytes count like any others
 * under the limit (two 4K streams hold 2 x 232 MB of 512: a third stream's caches may find less
 * room than without the layer -- raise the limit or set this option to 0 there).  Lowering the
 * option waits for the device and frees that layer only.  See sfrt_world_compact_cache_stats.
 * SFRT_OPT_PIXEL_CACHE (1 = default; 0 = off; 2 = every plain sfrt_world_render_band launch; other
 * values return SFRT_E_INVALID): the pixel layer on top of the texel cache and the compact layer.
 * At 1 it serves the launches it was measured to pay for by the project's rule -- not supersampled,
 * at most 64 spheres, no drawn texture ending beyond texel 65,535 of the atlas -- and at 2 also the
 * others (more spheres, larger atlases, supersampled worlds: gains the rule did not confirm).  What a launch that shades from those still
 * computes -- the texel, the brightness, the colour, the box filter when supersampled -- depends on
 * their state and on the textures' contents, which change only through sfrt_world_load_texture.
 * While that state stands still and no texture is loaded, the second consecutive
 * sfrt_world_render_band launch that reads the topmost of those layers is followed by a copy of the
 * band it wrote (4 bytes per output pixel, whatever the supersampling factor: 33.2 MB for a 4K
 * frame), and later launches are one copy of those pixels into the caller's band, whatever its
 * base and pitch: the same bytes and the same status.  Every sfrt_world_load_texture call, for any
 * slot and whether or not a sphere draws it, makes the next launch shade again from the layer
 * under this one -- the very next frame shows the new texels -- and the launch after it stores the
 * pixels again; a texture loaded every frame never fills the layer.  Only plain
 * sfrt_world_render_band launches take part (no planes, subsets, view batches or ray batches).
 * The bytes count against SFRT_OPT_HIT_CACHE_MB after the stream's other caches have theirs; where
 * they do not fit, launches stay on the layer under it.  Whatever drops or refills a cache under
 * it frees the stream's pixel layer first, so within a stream it never keeps a lower one from
 * filling; between streams its bytes count like any others under the limit.  Two 4K streams need
 * 2 x 265 MB at the default 512: the second stream's pixel layer does not fit and that stream stays
 * on its compact layer -- raise the limit to 531 to serve both.  Lowering the option waits for
 * the device and frees that layer only.  See sfrt_world_pixel_cache_stats. */
#define SFRT_OPT_CULL 1
#define SFRT_OPT_RAYS_PER_LANE 2
#define SFRT_OPT_TILE_ORDER 3
#define SFRT_OPT_SUPERSAMPLE 4
#define SFRT_OPT_RAY_CACHE_MB 5
#define SFRT_OPT_HIT_CACHE_MB 6
#define SFRT_OPT_TEXEL_CACHE 7
#define SFRT_OPT_COMPACT_TEXELS 8
#define SFRT_OPT_PIXEL_CACHE 9
SFRT_API int sfrt_world_set_option(sfrt_world* w, int option, int value);
/* The current value of any of the options above (SFRT_OPT_SUPERSAMPLE: the factor 1, 2 or 4). */
SFRT_API int sfrt_world_get_option(const sfrt_world* w, int option, int* value);
/* The ray cache's counters since the world was created (SFRT_OPT_RAY_CACHE_MB):
 * *cached_frames = launches that loaded their directions from a cache (the launch that
 * filled it included), *fills = launches preceded by a fill, *bytes = device memory the
 * world's caches hold now. */
SFRT_API int sfrt_world_ray_cache_stats(const sfrt_world* w, int64_t* cached_frames, int64_t* fills,
                                        int64_t* bytes);
/* *bytes = device memory the world's tile records hold now (32 bytes per tile of every filled
 * cache; 0 while SFRT_OPT_RAY_CACHE_MB is 0).  Not part of sfrt_world_ray_cache_stats' bytes. */
SFRT_API int sfrt_world_tile_record_bytes(const sfrt_world* w, int64_t* bytes);
/* The cull cache's counters since the world was created (SFRT_OPT_RAY_CACHE_MB): *fills =
 * launches preceded by a fill of the cull cache, *hits = launches that loaded their culling from
 * a cache filled earlier (the filling launch is not a hit), *bytes = device memory the world's
 * cull caches hold now.  Not part of sfrt_world_ray_cache_stats' bytes. */
SFRT_API int sfrt_world_cull_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits,
                                         int64_t* bytes);
/* The hit cache's counters since the world was created (SFRT_OPT_HIT_CACHE_MB): *fills = launches
 * that stored their march results, *hits = launches that shaded from stored results and did not
 * march (each also counts as a cached frame of sfrt_world_ray_cache_stats and a hit of
 * sfrt_world_cull_cache_stats), *bytes = device memory the world's hit caches hold now.  Not part
 * of the other caches' bytes. */
SFRT_API int sfrt_world_hit_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits,
                                        int64_t* bytes);
/* The texel cache's counters since the world was created (SFRT_OPT_TEXEL_CACHE): *fills = launches
 * that shaded from the hit cache and stored their texel indices, *hits = launches that shaded from
 * stored indices (each also counts as a hit of sfrt_world_hit_cache_stats and of the caches under
 * it), *bytes = device memory the world's texel caches hold now.  Counted against
 * SFRT_OPT_HIT_CACHE_MB, not part of sfrt_world_hit_cache_stats' bytes. */
SFRT_API int sfrt_world_texel_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits,
                                          int64_t* bytes);
/* The compact layer's counters since the world was created (SFRT_OPT_COMPACT_TEXELS): *fills =
 * launches that shaded from the texel cache and stored their 4-byte records, *hits = launches that
 * shaded from those (each also counts as a hit of sfrt_world_texel_cache_stats and of the caches
 * under it), *bytes = device memory the world's compact records hold now.  Counted against
 * SFRT_OPT_HIT_CACHE_MB, not part of the other caches' bytes. */
SFRT_API int sfrt_world_compact_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits,
                                            int64_t* bytes);
/* The pixel layer's counters since the world was created (SFRT_OPT_PIXEL_CACHE): *fills = launches
 * whose band was copied into the layer behind them, *hits = launches that were a copy out of it
 * (each also counts as a hit of every cache under it), *bytes = device memory the world's cached
 * pixels hold now.  Counted against SFRT_OPT_HIT_CACHE_MB, not part of the other caches' bytes. */
SFRT_API int sfrt_world_pixel_cache_stats(const sfrt_world* w, int64_t* fills, int64_t* hits,
                                          int64_t* bytes);

/* ---- stateless helpers ---- */
/* UpdateSpheres ordering of an array in place (SphereWorld.cpp:199-212). */
SFRT_API int sfrt_sort_spheres(sfrt_sphere* spheres, int count, const float cam_pos[3]);
/* deg * (PI / 180.0f) in binary32 (SphereWorld.cpp:72-73). */
SFRT_API float sfrt_deg_to_rad(float deg);
/* Exact pass threshold: for every binary32 s >= 0,
 * (radius - sqrtf(s) > 0.01f)  <=>  (s < sfrt_pass_threshold(radius)). */
SFRT_API float sfrt_pass_threshold(float radius);
SFRT_API const char* sfrt_error_string(int code);
SFRT_API int sfrt_version(void);
/* "release" for the shipped build; "diagnostic" for a -DSFRT_EXP timing/counter build
 * (writes wrong bytes by design) and "ab" for a build with extra flags (build-flag A/B).
 * bench.py refuses anything but "release". */
SFRT_API const char* sfrt_build_flavour(void);

/* ======================================================================
 * Band transfer packing (the exchange step of SURVEY 8e).  A frame
 * pixel's alpha is its texel's (SphereWorld.cpp:376-381, :109), and the
 * reference's textures hold alpha 0 or 255 only, so a band whose alphas are all
 * 0 or 255 packs losslessly into RGB plus one alpha bit: 3.125 bytes per pixel
 * on the wire instead of 4.  Format: B = ceil(pixels / 256), B * 800 bytes in two
 * planes: [0, 768*B) the RGB plane, pixel p's R, G, B at bytes 3p..3p+2 (zero past
 * the last pixel), then [768*B, 800*B) the alpha plane, the little-endian bit string
 * whose bit p is set when pixel p's alpha is 255 (zero past the last pixel).
 * Asynchronous on `hip_stream` of the device
 * current to the calling thread, which holds both buffers; dev_rgba 4-byte
 * and dev_packed 8-byte aligned.  Pixels whose alpha is neither 0 nor 255
 * unpack with alpha 0 -- pack only bands of a world whose
 * sfrt_world_alpha_binary is 1.
 * ====================================================================== */
SFRT_API int64_t sfrt_band_packed_bytes(int64_t pixels);  /* < 0: invalid */
SFRT_API int sfrt_band_pack(const void* dev_rgba, int64_t pixels, void* dev_packed, void* hip_stream);
SFRT_API int sfrt_band_unpack(const void* dev_packed, int64_t pixels, void* dev_rgba, void* hip_stream);
/* 1 when at least one texture is loaded and every texel of every loaded texture has
 * alpha 0 or 255 (so every pixel the world renders does), else 0.  With
 * SFRT_OPT_SUPERSAMPLE 2 or 4 a pixel's alpha is a mean of texel alphas, so it is 1 only
 * when, in addition, all those texels share one alpha (the mean of equal values). */
SFRT_API int sfrt_world_alpha_binary(const sfrt_world* w, int* binary);

/* ======================================================================
 * One frame over several GPUs of this node (BASELINE configs 4-5):
 * the reference caller is ONE C++ process (Source.cpp:17-28,47-52) that fills
 * one sf::Image; here it fills it on n GPUs.  The frame is split into
 * contiguous row bands, rank r = devices[r] renders rows [row0_r, row0_r +
 * rows_r) with the global row index (so the gathered frame is byte-identical
 * to a one-GPU render), and the bands travel to devices[0]:
 *   SFRT_MULTI_RCCL -- RCCL (librccl, loaded at create): one ncclGather for
 *                      equal bands, grouped ncclSend/ncclRecv otherwise;
 *   SFRT_MULTI_PEER -- hipMemcpyPeerAsync over xGMI (also serves a device
 *                      listed twice, which RCCL refuses);
 *   SFRT_MULTI_AUTO -- RCCL when the devices are distinct, else PEER.
 * Band transfers run on per-rank copy streams, so frame k's transfer overlaps
 * frame k+1's render (two band buffers per rank).  The scene setters below
 * apply to every rank's world; sfrt_multi_world gives a rank's world for
 * anything else (options).
 * ====================================================================== */
typedef struct sfrt_multi sfrt_multi;

#define SFRT_MULTI_AUTO 0
#define SFRT_MULTI_RCCL 1
#define SFRT_MULTI_PEER 2

SFRT_API int sfrt_multi_create(const int* hip_devices, int n, int transport, sfrt_multi** out);
/* The library behind SFRT_MULTI_RCCL: "" until the process's first RCCL context, then
 * "librccl.so.1" (or "librccl.so"), or "test:<path>" for a test transport; " (not loaded)"
 * is appended when it did not resolve.  SFRT_E_INVALID if it does not fit in `size`. */
SFRT_API int sfrt_multi_transport_library(char* buf, int size);
/* TEST ONLY: the RCCL C API from `library_path` instead of librccl (the tests' loopback
 * transport, tests/native/rccl_loopback.cpp, which accepts a device listed twice, so the
 * RCCL branch runs with n > 1 on one GPU).  Only before the process's first RCCL context
 * (else SFRT_E_INVALID); nothing in the environment selects it; reported by
 * sfrt_multi_transport_library. */
SFRT_API int sfrt_multi_use_test_transport(const char* library_path);
SFRT_API void sfrt_multi_destroy(sfrt_multi* m);
SFRT_API int sfrt_multi_count(const sfrt_multi* m, int* n, int* transport);
SFRT_API int sfrt_multi_world(sfrt_multi* m, int rank, sfrt_world** out);
SFRT_API int sfrt_multi_set_size(sfrt_multi* m, int width, int height);
SFRT_API int sfrt_multi_set_camera(sfrt_multi* m, const sfrt_camera* cam);
SFRT_API int sfrt_multi_load_texture(sfrt_multi* m, int slot, const uint8_t* rgba, int tex_w, int tex_h);
SFRT_API int sfrt_multi_set_spheres(sfrt_multi* m, const sfrt_sphere* spheres, int count);
SFRT_API int sfrt_multi_add_sphere(sfrt_multi* m, float x, float y, float z, float radius);
SFRT_API int sfrt_multi_update_spheres(sfrt_multi* m);
SFRT_API int sfrt_multi_set_sphere_textures(sfrt_multi* m, const int32_t* slots, int count);
SFRT_API int sfrt_multi_set_option(sfrt_multi* m, int option, int value);
/* Transfer format of the bands that cross a link (see "Band transfer packing"):
 * SFRT_TRANSFER_AUTO (default) packs when every rank's world is alpha-binary
 * (sfrt_world_alpha_binary), SFRT_TRANSFER_RGBA never packs, SFRT_TRANSFER_PACKED
 * always does (sfrt_multi_render fails with SFRT_E_INVALID on a world that is not
 * alpha-binary).  Packed bands travel by point-to-point transfers (RCCL) or peer
 * copies and are unpacked into the frame on devices[0]; the frame's bytes are the
 * same either way.  sfrt_multi_get_transfer: the setting and whether the last
 * render packed.  A supersampled world (SFRT_OPT_SUPERSAMPLE) whose textures are not
 * uniform in alpha is not alpha-binary: AUTO sends RGBA, PACKED fails the render. */
#define SFRT_TRANSFER_AUTO 0
#define SFRT_TRANSFER_RGBA 1
#define SFRT_TRANSFER_PACKED 2
SFRT_API int sfrt_multi_set_transfer(sfrt_multi* m, int format);
SFRT_API int sfrt_multi_get_transfer(sfrt_multi* m, int* format, int* last_packed);
/* Band heights: rows[r] for rank r (rank 0 first, sum = height at render time);
 * rows == NULL restores the default equal split (sfrt_multi_bands, factor 1). */
SFRT_API int sfrt_multi_set_bands(sfrt_multi* m, const int* rows, int n);
/* The partition helper (stateless, no device): row0/rows of n ranks for a frame
 * of `height` rows where rank 0 -- whose band never crosses a link -- gets about
 * `root_factor` times the rows of every other rank (their bands equal and
 * multiples of the 8-row tile); root_factor 1 = equal split
 * [r*H/n, (r+1)*H/n). */
SFRT_API int sfrt_multi_bands(int height, int n, float root_factor, int* row0, int* rows);
/* Cost-weighted partition (SURVEY 8e "Balance"; stateless, no device): rank 0 gets
 * `root_factor` shares of the frame's march cost sum(row_cost[0..height)), every
 * other rank one share; band edges on 8-row tile boundaries (or the last row).
 * row_cost: per-row work, e.g. from sfrt_world_row_costs / sfrt_multi_row_costs.
 * Invalid or all-zero costs give sfrt_multi_bands' partition. */
SFRT_API int sfrt_multi_cost_bands(const float* row_cost, int height, int n, float root_factor,
                                   int* row0, int* rows);
/* Per-row march cost of the whole frame from every rank's last band render
 * (sfrt_world_row_costs of each rank's world; costs[height]).  Synchronises. */
SFRT_API int sfrt_multi_row_costs(sfrt_multi* m, float* costs, int height);
/* Re-partition from the last frame's row costs: sfrt_multi_row_costs +
 * sfrt_multi_cost_bands + sfrt_multi_set_bands.  Call after a frame was rendered. */
SFRT_API int sfrt_multi_balance(sfrt_multi* m, float root_factor);
/* Render the whole width x height frame into `dev_frame` (device memory on
 * devices[0], pitch exactly width*4), asynchronously: every rank starts after
 * the work already queued on `hip_stream` (a stream of devices[0]; NULL = null
 * stream), and the frame is complete when `hip_stream` reaches the point after
 * this call.  sfrt_multi_check synchronises and reads every rank's status. */
SFRT_API int sfrt_multi_render(sfrt_multi* m, void* dev_frame, int64_t pitch_bytes, void* hip_stream);
SFRT_API int sfrt_multi_check(sfrt_multi* m);
/* UpdateImage(v, 0, 1, 0, 1) on n GPUs: the whole frame into the caller's host
 * RGBA8 buffer (width*height*4 bytes, pitch 4*width).  Synchronous. */
SFRT_API int sfrt_multi_update_image(sfrt_multi* m, uint8_t* pixels);

/* ======================================================================
 * Voxel World frame fill: drop-in for
 *   void World::UpdateImage(sf::Image* v, short ystart, short yadd,
 *                           short xstart, short xadd)
 *   (/root/reference/Raytracing/World.h:60, World.cpp:62-87; Raycast and
 *   LRaycast World.cpp:302-491) over a snapshot of the World state.
 * ====================================================================== */

/* struct Dynamic (World.h:25-38): the fields Raycast reads. */
typedef struct {
  float pos[3];
  float size[2];
  float r, g, b;
  float dist_to_camera;
  int32_t texture_id; /* dynTextures slot */
} sfrt_dynamic;

/* struct Light (World.h:40-47). */
typedef struct {
  float pos[3];
  float intensity, r, g, b;
  int32_t shadows;
} sfrt_light;

typedef struct sfrt_voxel sfrt_voxel;

#define SFRT_VOXEL_EMPTY (-32768)

/* A new voxel world: 320x180, Camera defaults of World.h:9-19 (pos 15.5, 1.9,
 * 15.5; fov 75/47 degrees converted like World.cpp:55-56), shadowDistance 16,
 * viewDistance 24 (World.h:70-71), no blocks/textures/objects/lights. */
SFRT_API int sfrt_voxel_create(int hip_device, sfrt_voxel** out);
SFRT_API void sfrt_voxel_destroy(sfrt_voxel* v);
SFRT_API int sfrt_voxel_set_size(sfrt_voxel* v, int width, int height);
SFRT_API int sfrt_voxel_set_camera(sfrt_voxel* v, const sfrt_camera* cam);
SFRT_API int sfrt_voxel_set_view(sfrt_voxel* v, float shadow_distance, float view_distance);
/* `blocks` (World.h:75) as a dense grid: texture_ids[(x*ny + y)*nz + z] is
 * Block::textureID (>= 0: textures[id]; < 0: colors[-id]) or SFRT_VOXEL_EMPTY;
 * lookups keep the map's (x<<20)+(y<<10)+z key semantics.  1 <= nx <= 2048, 1 <= ny, nz
 * <= 1024; the device copy is the key space itself, nx MiB of bytes (100 MiB for a
 * 100-wide world; 2 GiB for nx = 2048 whatever ny and nz are), rewritten by the first
 * frame after each call, stream-ordered on that frame's stream (no device-wide sync: it
 * waits on the device for the launches that read the old grid).  The call itself touches
 * no device memory: a grid the device cannot allocate fails that first frame call with
 * SFRT_E_HIP. */
SFRT_API int sfrt_voxel_set_blocks(sfrt_voxel* v, const int16_t* texture_ids, int nx, int ny, int nz);
SFRT_API int sfrt_voxel_load_texture(sfrt_voxel* v, int slot, const uint8_t* rgba, int w, int h);
SFRT_API int sfrt_voxel_load_dyn_texture(sfrt_voxel* v, int slot, const uint8_t* rgba, int w, int h);
SFRT_API int sfrt_voxel_set_colors(sfrt_voxel* v, const uint8_t* rgba, int count); /* colors[] */
/* `dyn` in list order (World.h:93) and `alights` in list order (World.h:95). */
SFRT_API int sfrt_voxel_set_dynamics(sfrt_voxel* v, const sfrt_dynamic* dyn, int count);
SFRT_API int sfrt_voxel_set_lights(sfrt_voxel* v, const sfrt_light* lights, int count);
/* The smallest squared distance dd >= 0 at which a light of this intensity adds nothing,
 * `intensity / dd - dd * 0.002f <= 0` in binary32 (World.cpp:425-426); 0 when no dd passes.
 * The kernel skips a light for a wave none of whose hit points is that close. */
SFRT_API float sfrt_voxel_light_dd_pass(float intensity);
/* World::UpdateImage into the caller's host RGBA8 frame; only addressed pixels written. */
SFRT_API int sfrt_voxel_update_image(sfrt_voxel* v, uint8_t* pixels, int ystart, int yadd, int xstart,
                                     int xadd);
/* Device row band [row0, row0+rows), asynchronous on hip_stream (NULL = null stream). */
SFRT_API int sfrt_voxel_render_band(sfrt_voxel* v, void* dev_pixels, int64_t pitch_bytes, int row0,
                                    int rows, void* hip_stream);
SFRT_API int sfrt_voxel_check(sfrt_voxel* v, void* hip_stream);

/* ---- the voxel frame fill's per-pixel planes: depth, cell, face, DDA steps ----
 * For pixel (i, j) of the world's width x height frame there are four optional planes of 4 bytes
 * per pixel, written by the same launch that writes the colour.  Line numbers are World.cpp's.
 *   face  (int32_t): what ended Raycast.
 *                    0: the loop of :324 ran out (the sf::Color::Black return of :452).
 *                    4: a billboard's opaque texel (the return at :373).
 *                    +-1, +-2, +-3: a block hit (:385).  The magnitude is colRay of that step
 *                    (1 = x, 2 = y, 3 = z; :329-349); the sign is that axis's dirXsign as
 *                    :312-314 set it, before :397-410 zero the others: -1 when the direction's
 *                    component is > 0, so the sign is the sign of the hit face's outward normal.
 *                    Defined for colour blocks (textureID < 0) as well.
 *   cell  (int32_t): block hit: the map key (posi.x << 20) + (posi.y << 10) + posi.z of :385,
 *                    computed in wrapping 32-bit arithmetic as the lookup does; it is >= 0 for
 *                    every hit.  Billboard: DI, the index into the list given to
 *                    sfrt_voxel_set_dynamics.  Nothing: -1.
 *   depth (float):   the binary32 value of `dist` when Raycast ends.  Block hit: tryDist as
 *                    assigned at :380 (the light loop's reuse of `dist` at :419 is not visible).
 *                    Billboard: d->distToCamera as assigned at :356.  Nothing: `dist` at loop
 *                    exit.  It is the reference's own ray parameter along the un-normalised
 *                    r->dir, which by :77 has unit component along the camera's horizontal
 *                    forward axis; nothing more is claimed of it.
 *   steps (int32_t): the number of times the body of the `while` at :324 was entered, the trip
 *                    that hit included; 0 when the first loop test fails.
 * Any plane may be NULL, but not all of them.  A non-NULL plane's pitch must be a multiple of 4
 * and at least 4*width; a NULL plane's pitch is ignored.  Violations return SFRT_E_INVALID with
 * nothing queued or written.  The plain calls' own checks apply unchanged (SFRT_E_EMPTY, band
 * bounds, sample-grid limits), and the plain calls keep their behaviour exactly.
 * Planes must not overlap each other or the colour target; that is the caller's duty.
 * A billboard's outcome depends on a texel's alpha, and an out-of-range texel read gives the
 * restatement's magenta with alpha 255: the planes are defined, and equal the reference's with
 * that texel, even when the status is SFRT_E_TEXEL.
 * With SFRT_OPT_SUPERSAMPLE S = 2 or 4 the colour is the box-filtered pixel as always, and the
 * planes are those of the output pixel's FIRST SAMPLE, sample pixel (S*i, S*j) of the
 * S*width x S*height frame, as the sphere planes are: no filtered or per-sample planes.
 * SFRT_OPT_TILE_ORDER is honoured exactly as sfrt_voxel_render_band honours it: an aux band and
 * a plain band of one stream share a chain.  sfrt_multi_*, the GLSL renderer and sfrt_world_*
 * are untouched. */
typedef struct {
  void* depth; int64_t depth_pitch_bytes;   /* float   per pixel, or NULL */
  void* cell;  int64_t cell_pitch_bytes;    /* int32_t per pixel, or NULL */
  void* face;  int64_t face_pitch_bytes;    /* int32_t per pixel, or NULL */
  void* steps; int64_t steps_pitch_bytes;   /* int32_t per pixel, or NULL */
} sfrt_voxel_aux_planes;
/* sfrt_voxel_render_band plus the planes (device memory on this world's device): same rows, same
 * global row index, same stream semantics; row r of a plane at plane + (r - row0) * its pitch.
 * The status is left to sfrt_voxel_check. */
SFRT_API int sfrt_voxel_render_band_aux(sfrt_voxel* v, void* dev_pixels, int64_t pitch_bytes,
                                        const sfrt_voxel_aux_planes* aux, int row0, int rows,
                                        void* hip_stream);
/* sfrt_voxel_update_image plus host planes of width*height elements (pitch 4*width), addressed
 * with the same strides; only addressed elements are written, in every plane.  A single-pixel
 * pick of (i, j) is xstart = i, xadd = width, ystart = j, yadd = height.  On SFRT_E_TEXEL the
 * call returns the code and writes neither `pixels` nor any plane, as sfrt_voxel_update_image
 * leaves `pixels` unwritten. */
SFRT_API int sfrt_voxel_update_image_aux(sfrt_voxel* v, uint8_t* pixels, float* depth, int32_t* cell,
                                         int32_t* face, int32_t* steps, int ystart, int yadd,
                                         int xstart, int xadd);

/* World::UpdateImage's pixel subsets in place in a device-resident frame: sfrt_world_render_subset
 * for the voxel world, with the same semantics -- `dev_frame` is the whole width x height frame,
 * only the addressed pixels' bytes (those of sfrt_voxel_update_image[_aux]) are written, in the
 * colour and in every non-NULL whole-frame plane; asynchronous on `hip_stream`, status through
 * sfrt_voxel_check; the same refusals; row-major, in no tile-order chain. */
SFRT_API int sfrt_voxel_render_subset(sfrt_voxel* v, void* dev_frame, int64_t pitch_bytes,
                                      int ystart, int yadd, int xstart, int xadd, void* hip_stream);
SFRT_API int sfrt_voxel_render_subset_aux(sfrt_voxel* v, void* dev_frame, int64_t pitch_bytes,
                                          const sfrt_voxel_aux_planes* aux, int ystart, int yadd,
                                          int xstart, int xadd, void* hip_stream);

/* ---- a batch of camera views of the voxel world in one launch ----
 * sfrt_world_render_views for the voxel world: each view a whole width x height frame from a
 * camera of its own into a device target of its own (sfrt_view, SFRT_MAX_VIEWS: the sphere
 * batch's), all views in one kernel launch.
 * Definition: with the world as it stands at the call, view k receives exactly the bytes that
 *   sfrt_voxel_set_camera(v, &views[k].cam);
 *   sfrt_voxel_set_dynamics(v, L, n);             -- with SFRT_VOXEL_VIEWS_DYNAMICS only: L = a copy
 *                                                    of the world's list after
 *                                                    sfrt_voxel_sort_dynamics(L, n, views[k].cam.pos)
 *   sfrt_voxel_render_band(v, views[k].dev_pixels, pitch_bytes, 0, height, s);
 * would write on a copy of that world (the aux call: sfrt_voxel_render_band_aux with planes[k]),
 * and the call writes no other byte.
 * What a camera owns in this renderer is more than its seven floats: the reference keeps
 * distToCamera and the ORDER of `dyn` per camera (World.cpp:226-231), and Raycast walks the list in
 * that order and stops at the first entry farther than the next block, so a list ordered for one
 * camera draws wrong billboards, or none, from another.  Without the flag every view uses the
 * world's list as it is (its order and its dist_to_camera values; only the angle term of :361 is
 * the view's own) -- right for views that share a position (cube-map faces).  With it each view
 * gets the list sorted for its own camera, always from the world's current list and never from
 * view k-1's, and a billboard's `cell` value in such a view indexes that view's sorted list
 * (recompute it with sfrt_voxel_sort_dynamics).
 * The lights are the world's list for every view: choosing `alights` per camera (World.cpp:233-240)
 * stays with the caller, as it is for a band.  view_distance and shadow_distance are the world's.
 * Whole frames only.
 * The world itself is left as it was: its camera, its dynamics list and that list's order, and
 * the tables a band has staged -- a sfrt_voxel_render_band after the batch with no setter in
 * between writes the bytes it wrote before.  A pending sfrt_voxel_set_blocks rewrite is carried out
 * by the call on its stream, as a band carries it out.
 * Asynchronous on `hip_stream` with sfrt_voxel_render_band's stream semantics; the texel bit of
 * every view goes into the world's status word (sfrt_voxel_check).  SFRT_OPT_SUPERSAMPLE is
 * honoured (planes: the first sample's, as above); the launch is row-major within a view and
 * view-major across views, so SFRT_OPT_TILE_ORDER has no influence and no chain is touched.
 * count == 0 returns SFRT_OK with nothing queued.  SFRT_E_INVALID, with nothing queued or written:
 * a NULL world or `views`, count < 0 or > SFRT_MAX_VIEWS, unknown flag bits, pitch_bytes not a
 * multiple of 4 or below 4*width, a NULL or not 4-byte-aligned dev_pixels or a camera
 * sfrt_voxel_set_camera would refuse in any view, (aux) NULL `planes`, an entry with all four
 * planes NULL or with a pitch sfrt_voxel_render_band_aux would refuse, a sample grid a band would
 * refuse, or a grid the device cannot be given in one launch (more than 2^31 - 1 tiles over all
 * views, or more than 2^26 - 1 tiles in one).  SFRT_E_EMPTY as for a band.  Targets (and planes)
 * that overlap are the caller's responsibility. */
#define SFRT_VOXEL_VIEWS_DYNAMICS 1   /* flags bit 0: distToCamera and the list order per view */
SFRT_API int sfrt_voxel_render_views(sfrt_voxel* v, const sfrt_view* views, int count,
                                     int64_t pitch_bytes, int flags, void* hip_stream);
SFRT_API int sfrt_voxel_render_views_aux(sfrt_voxel* v, const sfrt_view* views,
                                         const sfrt_voxel_aux_planes* planes /* count entries */,
                                         int count, int64_t pitch_bytes, int flags, void* hip_stream);
/* The per-camera part of World::UpdateDynamics for a list, in place (a pure host function, like
 * sfrt_sort_spheres): every dist_to_camera becomes the binary32 value of World.cpp:226-227,
 * sqrtf(to.x*to.x + to.z*to.z) with to = pos - cam_pos (products and sum rounded one by one), and
 * the list is then ordered by insertion from the front: element i goes before the first already
 * placed element whose distance is greater, by the `<` of World.cpp:229 (a NaN distance is never
 * greater and never smaller: such an element stays behind everything placed before it).  That is
 * a stable ascending sort.  It is NOT the reference's one pass: World.cpp:229-231 swaps each
 * element at most once with its predecessor per frame, one bubble pass, and reaches this order
 * only after enough frames with the camera at rest -- this order is that iteration's fixed point,
 * the list a camera that has stood still sees.  A caller that wants the reference's transient
 * order does its passes itself and renders without the flag.
 * SFRT_E_INVALID for count < 0 or a NULL pointer with count > 0. */
SFRT_API int sfrt_voxel_sort_dynamics(sfrt_dynamic* dyn, int count, const float cam_pos[3]);

/* ---- batched ray queries: World::Raycast (World.cpp:302-453) for caller-supplied rays ----
 * sfrt_voxel_cast_rays[_device] runs Raycast for ray q of a batch.  Line numbers are World.cpp's.
 * `dirs` holds 3 floats per ray, used as r->dir VERBATIM: the voxel Raycast never normalises, and
 * `depth` is the reference's own ray parameter along that direction, as the depth plane above
 * documents it.  `yscales` holds one float per ray, r->yscale; NULL means 1.0f for every ray.
 * origins == NULL is the reference: pos = cam.pos (:305), snapshotted at the call, and the
 * billboard loop of :353-378 runs, with atan2f(dir.z, dir.x) of VAngleXZ evaluated per ray by
 * sfrt_math::atan2f.
 * origins != NULL, 3 floats per ray: cam.pos of :305 is replaced by the ray's origin, and the
 * billboard list is NOT VISITED, as if `dyn` were empty: distToCamera and
 * VNormalizeXZ(d->pos - cam.pos) are camera quantities and have no meaning for another origin.
 * Blocks, lights and shadow rays are unchanged: the hit block is shaded by :386-450 as for a
 * pixel, shadowDistance compared with the ray's own tryDist.
 * Outputs.  depth, cell, face and steps are exactly as the planes of sfrt_voxel_render_band_aux
 * define them (face never 4 with origins given).  pos depends on how the ray ended: block hit,
 * pos as assigned at :381, before :396-408 move it off the wall; billboard, pos after :357 for
 * the billboard that returned; nothing, pos at loop exit.  rgba is r->c.  rgba == NULL skips the
 * shading of a block hit entirely -- no block texel, no light loop, no shadow rays: the picking
 * path does not pay for shading.  A billboard's alpha test still reads its texel then, so the
 * texel status bit can still be set.
 * A direction component of 0 is valid (the reference's own axis-parallel column has one) and
 * marches as the frame kernels march it.  Arithmetic is binary32, round to nearest, no
 * contraction, with correctly rounded / and sqrt, and the float -> int conversions of the
 * reference's x86-64 build, as in the frame fill.
 * An invalid ray is one with any non-finite component of dir, origin or yscale.  It is decided
 * per ray before the march and never marched.  It gets face = 0, cell = -1, steps = 0, and every
 * other requested output is all-zero bytes.  It changes no other ray's result and sets no status
 * bit.
 * Return codes.  count == 0 returns SFRT_OK and writes nothing.  SFRT_E_INVALID, with nothing
 * queued or written, for: a NULL world; NULL dirs; a NULL output record; count < 0 or count >
 * 2^31-1; all six outputs NULL; a non-NULL pointer that is not 4-byte aligned.  SFRT_E_EMPTY when
 * there are no blocks, as the frame calls give it.  Overlapping buffers are the caller's
 * responsibility.
 * Status.  The only status bit is the frame fill's texel bit.  The device call is asynchronous
 * on hip_stream and leaves it to sfrt_voxel_check(v, hip_stream).  The host call returns the
 * code; on SFRT_E_TEXEL it writes no output, as sfrt_voxel_update_image_aux.
 * Shared state.  A batch counts as a frame call for the deferred grid upload of
 * sfrt_voxel_set_blocks and for the staged dynamics, lights and texture tables.  Calls serialise
 * on the world's mutex; scene, camera and view distances are snapshotted at the call.
 * SFRT_OPT_SUPERSAMPLE and SFRT_OPT_TILE_ORDER are ignored: the call joins no tile-order chain
 * and leaves the recorded tile costs alone.  The host calls stage through one device buffer and
 * one pinned buffer per world, grown on demand. */
typedef struct {          /* every member: one element per ray, or NULL; not all NULL */
  float*   pos;           /* 3 floats per ray, packed x,y,z (12 B per ray) */
  float*   depth;
  int32_t* cell;          /* -1: nothing hit, or an invalid ray */
  int32_t* face;          /* 0: nothing hit, or an invalid ray */
  int32_t* steps;         /* 0: invalid ray */
  uint8_t* rgba;          /* 4 bytes per ray: r->c */
} sfrt_voxel_ray_hits;
/* device memory on the world's device, asynchronous on hip_stream; status via sfrt_voxel_check */
SFRT_API int sfrt_voxel_cast_rays_device(sfrt_voxel* v, const float* dev_dirs, const float* dev_yscales,
                                         const float* dev_origins, int64_t count,
                                         const sfrt_voxel_ray_hits* dev_out, void* hip_stream);
/* host memory, synchronous */
SFRT_API int sfrt_voxel_cast_rays(sfrt_voxel* v, const float* dirs, const float* yscales,
                                  const float* origins, int64_t count, const sfrt_voxel_ray_hits* out);

/* ---- batched occlusion queries: World::LRaycast (World.cpp:455-491) for caller-supplied rays ----
 * Ray q is LRaycast with r->pos = origins[3q..], r->dir = dirs[3q..] verbatim (the reference
 * passes a normalised one) and r->maxDist = max_dists[q].
 *   free  (int32_t): 1 where LRaycast returns true; 0 where it returns false -- a block, or the
 *                    trip limit max(maxDist*2, 20) of :473 before maxDist; -1 for an invalid ray.
 *   steps (int32_t): the number of times the body of the `for` at :475 was entered, the trip that
 *                    returned false included; 0 for an invalid ray.
 * Either output may be NULL, but not both.  A negative or zero max_dist is valid: the loop never
 * runs and the answer is 1, as in the reference.  A zero direction component is valid.
 * A ray is invalid when any component of origin or dir, or max_dist itself, is not finite, or
 * when max_dist > SFRT_VOXEL_MAX_SHADOW_DIST: without a bound one caller value of 1e9 would keep
 * a wave busy for 2e9 trips; 4096 covers viewDistance values far beyond the reference's 24.  An
 * invalid ray is never marched and changes no other ray's result.
 * No billboards, no textures, no status bits.  count == 0 returns SFRT_OK and writes nothing;
 * SFRT_E_INVALID, with nothing queued or written, for a NULL world, NULL origins, dirs or
 * max_dists, count < 0 or count > 2^31-1, both outputs NULL, or a non-NULL pointer that is not
 * 4-byte aligned; SFRT_E_EMPTY when there are no blocks.  Shared state, snapshots, the mutex and
 * the host call's staging are sfrt_voxel_cast_rays'. */
#define SFRT_VOXEL_MAX_SHADOW_DIST 4096.0f
SFRT_API int sfrt_voxel_cast_shadow_rays_device(sfrt_voxel* v, const float* dev_origins,
                                                const float* dev_dirs, const float* dev_max_dists,
                                                int64_t count, int32_t* dev_free, int32_t* dev_steps,
                                                void* hip_stream);
SFRT_API int sfrt_voxel_cast_shadow_rays(sfrt_voxel* v, const float* origins, const float* dirs,
                                         const float* max_dists, int64_t count, int32_t* free_,
                                         int32_t* steps);

/* SFRT_OPT_TILE_ORDER as for sfrt_world, but off (0) by default here: render_band with 1
 * dispatches 8x8 tiles longest-first by the DDA + shadow steps of two frames back (same
 * bytes; measured 1-6% slower on the voxel worlds).
 * SFRT_OPT_SUPERSAMPLE (1 = default, today's frame byte for byte; 2 or 4; any other value
 * returns SFRT_E_INVALID and changes nothing): S x S samples per pixel, box-filtered inside the
 * kernel by the rule stated for sfrt_world (each of the four output bytes, alpha included, is
 * (sum of the S*S sample bytes + S*S/2) >> log2(S*S)).  The samples of output pixel (i, j) are
 * the pixels (S*i + k, S*j + l), 0 <= k, l < S, of World::UpdateImage at width S*width and
 * height S*height (World.cpp:64-87 evaluated with those sizes: hIncreaseBy = cam.fovH /
 * (S*width), vIncreaseBy = cam.fovV / (S*height)), each traced and shaded to RGBA8 as always
 * (Raycast, LRaycast, billboards, lights; the texel status bit per sample).  The strides of
 * sfrt_voxel_update_image address output pixels and only those are written; row0, rows, the
 * pitch and the buffer of sfrt_voxel_render_band are in output pixels and bands tile the frame
 * byte for byte.  Voxel frames hold alpha 0 as well as 255, so averaged alphas take values in
 * between.  A frame call returns SFRT_E_INVALID, with nothing queued or written, when S*width
 * or S*height does not fit an int or the sample grid has more tiles than one launch takes. */
SFRT_API int sfrt_voxel_set_option(sfrt_voxel* v, int option, int value);
/* The stored SFRT_OPT_TILE_ORDER (0, 1 or 2) or SFRT_OPT_SUPERSAMPLE (the factor 1, 2 or 4);
 * any other option returns SFRT_E_INVALID. */
SFRT_API int sfrt_voxel_get_option(const sfrt_voxel* v, int option, int* value);

/* ======================================================================
 * GLSL renderer: drop-in for the live GPU path
 *   world.shader.setUniform(...)                (SphereWorld.cpp:214-238,
 *                                                Source.cpp:143-146)
 *   rt.draw(sp, &world.shader)                  (Source.cpp:150-153)
 * i.e. rayShader.frag (/root/reference/Raytracing/rayShader.frag:1-179) run
 * once per pixel of a width x height render target.  Semantics the shader
 * leaves to the driver are fixed in DESIGN.md section 4b.
 * ====================================================================== */

#define SFRT_GLSL_MAX_SPHERES 100 /* uniform vec4 spheres[100] (rayShader.frag:6-8) */

/* The shader's uniforms (rayShader.frag:1-11); `ground` is set separately. */
typedef struct {
  float campos[3];
  float rotation[2]; /* (cam.rotation, cam.hrotation) */
  float fov[2];      /* (fovH, fovV) in radians */
  float size[2];     /* render-target size */
  int32_t sphere_count, all_spheres_count, light_count;
  float spheres[SFRT_GLSL_MAX_SPHERES][4]; /* xyz, radius: walls, lights, ospheres */
  float uvs[SFRT_GLSL_MAX_SPHERES][4];
  float lights[SFRT_GLSL_MAX_SPHERES][4];
} sfrt_glsl_uniforms;

typedef struct sfrt_glsl sfrt_glsl;

/* A new shader instance: all uniforms zero (GLSL's initial uniform values),
 * no ground texture. */
SFRT_API int sfrt_glsl_create(int hip_device, sfrt_glsl** out);
SFRT_API void sfrt_glsl_destroy(sfrt_glsl* g);
/* setUniform("ground", t) with t.setRepeated(true), t.generateMipmap()
 * (SphereWorld.cpp:52-57): RGBA8 rows, power-of-two sides. */
SFRT_API int sfrt_glsl_set_ground(sfrt_glsl* g, const uint8_t* rgba, int w, int h);
SFRT_API int sfrt_glsl_set_uniforms(sfrt_glsl* g, const sfrt_glsl_uniforms* u);
SFRT_API int sfrt_glsl_get_uniforms(sfrt_glsl* g, sfrt_glsl_uniforms* u);
/* sf::Shader::setUniform by name: "campos" (3 floats), "rotation", "fov",
 * "size" (2), "spheres[k]", "uvs[k]", "lights[k]" (4); ints "sphereCount",
 * "allSpheresCount", "lightCount".  Unknown names -> SFRT_E_INVALID. */
SFRT_API int sfrt_glsl_set_uniform(sfrt_glsl* g, const char* name, const float* v, int n);
SFRT_API int sfrt_glsl_set_uniform_int(sfrt_glsl* g, const char* name, int value);
/* rt.draw: rows [row0, row0+rows) of a width x height target into device
 * memory (row 0 = top of the image, as rt.getTexture().copyToImage()),
 * asynchronous on hip_stream (NULL = null stream). */
SFRT_API int sfrt_glsl_draw(sfrt_glsl* g, void* dev_pixels, int width, int height,
                            int64_t pitch_bytes, int row0, int rows, void* hip_stream);
/* rt.draw + rt.getTexture().copyToImage() into a host RGBA8 buffer (synchronous). */
SFRT_API int sfrt_glsl_draw_image(sfrt_glsl* g, uint8_t* pixels, int width, int height);
SFRT_API int sfrt_glsl_check(sfrt_glsl* g, void* hip_stream);

/* ---- the draw's per-pixel planes: depth, sphere index, march steps ----
 * sfrt_glsl_draw / sfrt_glsl_draw_image plus the three optional planes of sfrt_aux_planes (4 bytes
 * per pixel, each with its own pitch), written by the same launch that writes the colour:
 *   depth  (float):   totalDist after rayShader.frag:117 -- the wall distance of the wall pass
 *                     (:71-85) for a wall pixel, ballDist for a ball pixel -- before the
 *                     brightness (:128) and the fog (:156) use it.
 *   sphere (int32_t): drawSphere after :118, an index into the spheres[] uniform: walls are
 *                     < sphereCount, then the lights, then the ospheres.
 *   steps  (int32_t): the trips of the metaball loop :94-112 (0 when it never ran), the count the
 *                     adaptive tile order uses as a tile's cost.
 * Any plane may be NULL, but not all three.  SFRT_E_INVALID, with nothing queued or written, when
 * all three are NULL or (draw_aux) a non-NULL plane's pitch is not a multiple of 4 or is below
 * 4*width; a NULL plane's pitch is ignored.  The plain calls' own argument checks apply unchanged
 * and the colour bytes are exactly the plain calls'.  Row r of a plane is at plane + (r - row0) *
 * its pitch.  With SFRT_OPT_SUPERSAMPLE S = 2 or 4 the colour is box-filtered as always and the
 * planes describe the output pixel's FIRST SAMPLE, fragment (S*i, S*row) of the S*width x S*height
 * target: point-sampled; no filtered, minimum or per-sample depth.  A pixel whose march hit the
 * cap (SFRT_E_MARCH_LIMIT) is unspecified, as its colour is.  Planes must not overlap each other
 * or the colour target.  sfrt_glsl_draw_aux honours SFRT_OPT_TILE_ORDER and joins its stream's
 * tile chain exactly as sfrt_glsl_draw does (the two share one chain); sfrt_glsl_draw_image_aux is
 * row-major with host planes of width*height elements.  Table-slot reuse, ground ordering and the
 * status word are the plain draw's. */
SFRT_API int sfrt_glsl_draw_aux(sfrt_glsl* g, void* dev_pixels, int width, int height,
                                int64_t pitch_bytes, const sfrt_aux_planes* aux,
                                int row0, int rows, void* hip_stream);
SFRT_API int sfrt_glsl_draw_image_aux(sfrt_glsl* g, uint8_t* pixels, float* depth,
                                      int32_t* sphere, int32_t* steps, int width, int height);

/* ---- batched ray queries: the shader's Raycast(campos, dir, 1) (rayShader.frag:63-161) ----
 * Ray q has the direction dirs[3q..3q+2], un-normalised; :65 normalises it as it does a
 * fragment's.  EVERY RAY STARTS AT campos.  There are no per-ray origins, on purpose: the
 * shader's own Raycast marches the metaballs from campos whatever `pos` it is given (:95, :119),
 * and the tables a draw prepares on the host (the first wall that holds campos, the -0.0 rule,
 * the wall cull's margin, the shadow cones' bound) are per campos.  rotation, fov, size,
 * SFRT_OPT_SUPERSAMPLE and SFRT_OPT_TILE_ORDER do not influence a batch (rotation, fov and size
 * are not even validated for it); a batch joins no tile chain and leaves the recorded tile costs
 * alone.  The uniforms are snapshotted at the call.
 * Outputs (sfrt_ray_hits, each NULL or one element per ray, not all NULL):
 *   pos    pos after :119: the wall pass's point for a wall hit, campos + dir * ballDist for a ball;
 *   depth, sphere, steps   as the planes above;
 *   rgba   the fragment's colour through the framebuffer's unorm8 conversion, alpha 255.
 *          rgba == NULL skips the shading (:123-158) entirely.
 * An invalid ray.  A ray is invalid when any direction component is not finite, or when
 * s = (dx*dx + dy*dy) + dz*dz is not a finite normal number.  That covers zero, underflow and
 * overflow.  It is decided per ray before the march.  It is never marched.  It gets sphere = -1,
 * and every other requested output is all-zero bytes.  It must not change any other ray's result.
 * It sets no status bit.
 * Return codes and edge cases.  count == 0 returns SFRT_OK and writes nothing.  SFRT_E_INVALID,
 * with nothing queued or written, for: a NULL shader; NULL dirs; a NULL output record; count < 0
 * or count > 2^31-1; all five outputs NULL; a non-NULL pointer that is not 4-byte aligned; uniforms
 * a draw would refuse (counts, bounds of campos and the sphere tables).  SFRT_E_NO_TEXTURE only
 * when rgba is requested: a shader without a ground can still answer pos, depth, sphere and steps.
 * Overlapping buffers are the caller's responsibility.
 * Status.  The march-cap bit is the draw's own.  The device call leaves it to
 * sfrt_glsl_check(g, hip_stream); the host call returns the code with the outputs written, as
 * sfrt_glsl_draw_image does.  Calls serialise on the shader's mutex. */
/* device memory on the shader's device, asynchronous on hip_stream */
SFRT_API int sfrt_glsl_cast_rays_device(sfrt_glsl* g, const float* dev_dirs, int64_t count,
                                        const sfrt_ray_hits* dev_out, void* hip_stream);
/* host memory, synchronous */
SFRT_API int sfrt_glsl_cast_rays(sfrt_glsl* g, const float* dirs, int64_t count,
                                 const sfrt_ray_hits* out);

/* ---- a batch of camera views of the shader in one launch ----
 * sfrt_world_render_views for the GLSL renderer: each view a whole width x height frame from a
 * camera of its own into a device target of its own (sfrt_view, SFRT_MAX_VIEWS: the sphere
 * batch's), all views in one kernel launch, with one host table build and one upload.
 * Definition: with the shader as it stands at the call, view k receives exactly the bytes that
 *   sfrt_glsl_set_uniform(g, "campos",   views[k].cam.pos, 3);
 *   sfrt_glsl_set_uniform(g, "rotation", (cam.rotation, cam.hrotation), 2);
 *   sfrt_glsl_set_uniform(g, "fov",      (cam.fov_h, cam.fov_v), 2);
 *   sfrt_glsl_draw(g, views[k].dev_pixels, width, height, pitch_bytes, 0, height, s);
 * would write on a copy of that shader (the aux call: sfrt_glsl_draw_aux with planes[k]), and the
 * call writes no other byte.  The `size` uniform and every scene uniform (the counts, spheres, uvs,
 * lights, the ground) are the shader's own for all views.  Whole frames only.  `flags` must be 0:
 * the shader sorts nothing per camera, so no flag is defined.
 * The shader itself is left as it was: its uniform block (sfrt_glsl_get_uniforms returns the same
 * bytes), the tables a draw has staged and the tile chains -- a sfrt_glsl_draw after the batch with
 * no setter in between writes the bytes it wrote before and stages nothing again.
 * Asynchronous on `hip_stream` with sfrt_glsl_draw's stream semantics; the march-cap bit of every
 * view goes into the shader's status word (sfrt_glsl_check).  SFRT_OPT_SUPERSAMPLE is honoured
 * (`size` scaled by S as in a draw; planes: the first sample's, as above); the launch is row-major
 * within a view and view-major across views, so SFRT_OPT_TILE_ORDER has no influence, no chain is
 * joined and the recorded tile costs stay.
 * count == 0 returns SFRT_OK with nothing queued.  SFRT_E_INVALID, with nothing queued or written:
 * a NULL shader or `views`, count < 0 or > SFRT_MAX_VIEWS, flags != 0, a width or height
 * sfrt_glsl_draw would refuse, pitch_bytes not a multiple of 4 or below 4*width, a NULL or not
 * 4-byte-aligned dev_pixels in any view, a camera whose pos, rotation, hrotation, fov_h or fov_v a
 * draw would refuse as uniforms in any view, scene uniforms a draw would refuse, (aux) NULL
 * `planes`, an entry with all three planes NULL or with a pitch sfrt_glsl_draw_aux would refuse, or
 * a grid the device cannot be given in one launch (more than 2^31 - 1 tiles over all views, or more
 * than 2^26 - 1 tiles in one, counted on the sample grid when supersampled).  SFRT_E_NO_TEXTURE
 * when there is no ground.  Calls serialise on the shader's mutex.  Targets (and planes) that
 * overlap are the caller's responsibility. */
SFRT_API int sfrt_glsl_render_views(sfrt_glsl* g, const sfrt_view* views, int count,
                                    int width, int height, int64_t pitch_bytes,
                                    int flags, void* hip_stream);
SFRT_API int sfrt_glsl_render_views_aux(sfrt_glsl* g, const sfrt_view* views,
                                        const sfrt_aux_planes* planes /* count entries */,
                                        int count, int width, int height,
                                        int64_t pitch_bytes, int flags, void* hip_stream);

/* SFRT_OPT_TILE_ORDER as for sfrt_world, on (1) by default: sfrt_glsl_draw dispatches 8x8
 * tiles longest-first by the metaball-march steps of two frames back (same bytes; 1-6 % faster
 * on the round-4 kernel); 0 = row-major.  sfrt_glsl_draw_image is row-major.
 * SFRT_OPT_SUPERSAMPLE (1 = default, today's frame byte for byte; 2 or 4; any other value
 * returns SFRT_E_INVALID and changes nothing): S x S samples per pixel, box-filtered inside the
 * kernel by the rule stated for sfrt_world.  The samples are the fragments of an S*width x
 * S*height render target: the `size` uniform is replaced by (S*size[0], S*size[1]) (exact in
 * binary32), every other uniform is unchanged, and sample (a, b), b counted from the top, has
 * gl_FragCoord = (a + 0.5, (S*height - 1 - b) + 0.5).  width, height, row0, rows and the pitch
 * of sfrt_glsl_draw and sfrt_glsl_draw_image stay in output pixels; output alpha stays 255.
 * A draw returns SFRT_E_INVALID, with nothing queued or written, when S*width or S*height
 * reaches 2^24 or S*size is beyond the uniforms' bound. */
SFRT_API int sfrt_glsl_set_option(sfrt_glsl* g, int option, int value);
/* The stored SFRT_OPT_TILE_ORDER (0, 1 or 2) or SFRT_OPT_SUPERSAMPLE (the factor 1, 2 or 4);
 * any other option returns SFRT_E_INVALID. */
SFRT_API int sfrt_glsl_get_option(const sfrt_glsl* g, int option, int* value);

/* ======================================================================
 * Asset pipeline: PNG -> RGBA8 as sf::Image::loadFromFile
 * (SFML 2.4.2 / stb_image, 4 channels) decodes the reference's textures
 * (SphereWorld.cpp:52-53, World.cpp:40-45).  Host-only; no device needed.
 * ====================================================================== */
SFRT_API int sfrt_png_info(const uint8_t* data, int64_t len, int* width, int* height);
/* rgba: capacity bytes >= width*height*4 (query with sfrt_png_info). */
SFRT_API int sfrt_png_decode(const uint8_t* data, int64_t len, uint8_t* rgba, int64_t capacity,
                             int* width, int* height);

#ifdef __cplusplus
}
#endif
#endif /* SFRT_H */
