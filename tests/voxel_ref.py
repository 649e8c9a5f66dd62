"""World::UpdateImage / Raycast / LRaycast restated in numpy binary32 (test helper).

The voxel oracle (oracle/voxelworld_oracle.c) hands back colours only.  The per-pixel planes of
sfrt_voxel_render_band_aux (include/sfrt.h: depth, cell, face, steps) need the march's
intermediates, so this module restates, for all rays of a frame at once,

  * the ray setup of World::UpdateImage (World.cpp:62-87): `frame_rays`;
  * World::Raycast (World.cpp:302-453), keeping what ended each ray: `render`;
  * World::LRaycast (World.cpp:455-491) for the shadow rays of the colour: `_lraycast`.

Every operation is a float32 numpy operation in the reference's operand order (numpy neither
contracts nor reassociates; + - * / and sqrt are correctly rounded); sinf / cosf / atan2f are the
host libm's through ctypes, the functions the reference calls.  The float -> integer conversions
are those of the reference's x86-64 build (to_i32, to_u32, to_u8: out of range and NaN give
INT_MIN / 0), the block lookup keeps the map key's wrapping semantics (block_at) and a texel read
outside a texture gives magenta with alpha 255 and is counted, as the oracle does.

The restatement is trusted only because tests/test_voxel_ref.py pins its colour frame to the
oracle's bytes; the planes are by-products of the same march.  `shade=False` skips the light
loop (the planes and the texel count do not depend on it) and returns no colour.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
EMPTY = -32768
PI = F(3.1415926535)     # World.h:5
PI2 = F(6.28318530718)   # World.h:6
INT_MIN = np.int32(-2147483648)
MAGENTA = np.array([255, 0, 255, 255], dtype=np.uint8)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name, _n in (("sinf", 1), ("cosf", 1), ("atan2f", 2)):
    _fn = getattr(_libm, _name)
    _fn.argtypes = [ctypes.c_float] * _n
    _fn.restype = ctypes.c_float


def _map(name, *args):
    fn = getattr(_libm, name)
    arrs = np.broadcast_arrays(*[np.asarray(a, dtype=F) for a in args])
    out = np.fromiter((fn(*(float(v) for v in vs)) for vs in zip(*(a.ravel() for a in arrs))),
                      dtype=F, count=arrs[0].size)
    return out.reshape(arrs[0].shape)


def to_i32(f):
    """float -> int as cvttss2si: truncation; INT_MIN when out of range or NaN."""
    f = np.asarray(f, dtype=F)
    ok = (f > F(-2147483648.0)) & (f < F(2147483648.0))
    return np.where(ok, np.where(ok, f, F(0)).astype(np.int32), INT_MIN)


def to_u32(f):
    """float -> unsigned as x86-64 g++ emits it: 64-bit cvttss2si, low 32 bits (as int64)."""
    f = np.asarray(f, dtype=F)
    ok = (f > F(-9.2233720368547758e18)) & (f < F(9.2233720368547758e18))
    return np.where(ok, f, F(0)).astype(np.int64) & 0xffffffff


def to_u8(f):
    """float -> sf::Uint8: cvttss2si to int, low byte."""
    return (to_i32(f).astype(np.int64) & 0xff).astype(np.uint8)


def _min255(v):
    """std::min(v, 255.0f): (255.0f < v) ? 255.0f : v, NaN stays NaN."""
    return np.where(F(255.0) < v, F(255.0), v)


def block_key(x, y, z):
    """(x << 20) + (y << 10) + z in wrapping 32-bit arithmetic, as a signed value (int64)."""
    k = ((x.astype(np.int64) << 20) + (y.astype(np.int64) << 10) + z.astype(np.int64)) & 0xffffffff
    return np.where(k >= 1 << 31, k - (1 << 32), k)


def block_at(blocks, x, y, z):
    """blocks.contains(key) (World.cpp:385, 476): (present, textureID, key).  The map's keys are
    those of the grid's occupied cells: present iff the key is non-negative and decodes to one."""
    key = block_key(x, y, z)
    nx, ny, nz = blocks.shape
    cx, cy, cz = key >> 20, (key >> 10) & 1023, key & 1023
    ok = (key >= 0) & (cx < nx) & (cy < ny) & (cz < nz)
    ids = np.full(key.shape, EMPTY, dtype=np.int16)
    ids[ok] = blocks[cx[ok], cy[ok], cz[ok]]
    return ids != EMPTY, ids, key


def _texel(tex, x, y):
    """The texel at (x, y) (unsigned, as int64): (rgba (n, 4) uint8, outside (n,) bool)."""
    n = x.shape[0]
    if tex is None or tex[0] is None:
        return np.broadcast_to(MAGENTA, (n, 4)).copy(), np.ones(n, dtype=bool)
    data, w, h = tex
    data = np.asarray(data, dtype=np.uint8).reshape(-1, 4)
    idx = (x + y * w) & 0xffffffff
    bad = idx >= ((w * h) & 0xffffffff)
    out = np.broadcast_to(MAGENTA, (n, 4)).copy()
    out[~bad] = data[idx[~bad]]
    return out, bad


def _slot(lst, k):
    return lst[k] if 0 <= k < len(lst) else None


def _tex_dims(tex):
    return (F(0), F(0)) if tex is None or tex[0] is None else (F(np.uint32(tex[1])), F(np.uint32(tex[2])))


def frame_rays(scene, width, height):
    """World.cpp:62-87: per column i (dir.x, dir.z, atan2f(dir.z, dir.x)), per row j (dir.y,
    yscale), all float32."""
    fov_h, fov_v = F(scene.fov_h), F(scene.fov_v)
    rot, hrot = F(scene.rotation), F(scene.hrotation)
    v_start = fov_v / F(2)
    v_inc = fov_v / F(height)
    v_off = _map("sinf", hrot)
    h_start = rot - fov_h / F(2)
    h_inc = fov_h / F(width)
    with np.errstate(all="ignore"):
        hray = h_start + h_inc * np.arange(width).astype(F)
        fix = _map("cosf", rot - hray)               # "Fix distortion on edges", :77
        dx = _map("sinf", hray) / fix
        dz = _map("cosf", hray) / fix
        vray = v_start - np.arange(height).astype(F) * v_inc
        yscale = _map("cosf", hrot + vray)
        dy = v_off + _map("sinf", vray)
        at = _map("atan2f", dz, dx)                  # VAngleXZ's ray term, :272
    for a in (hray, fix, dx, dz, vray, yscale, dy, at):
        assert a.dtype == F
    return dx, dz, at, dy, yscale


def _dda_terms(d):
    add = np.where(d > 0, F(1), F(0))
    sign = np.where(d > 0, F(-1), F(1))
    return add, sign, np.abs(d)


def _lraycast(blocks, pos, d, max_dist):
    """World::LRaycast, World.cpp:455-491, for n rays: True where the path to the light is free."""
    n = pos.shape[0]
    pos = pos.copy()
    dist = np.zeros(n, dtype=F)
    pi = to_i32(pos)
    add, sign, ln = _dda_terms(d)
    m2 = max_dist * F(2)
    max_iter = to_u32(np.where(m2 < F(20.0), F(20.0), m2))                 # :473
    blocked = np.zeros(n, dtype=bool)
    i = np.zeros(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    while True:
        live &= (i < max_iter) & (dist < max_dist)                          # :475
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        hit, _, _ = block_at(blocks, pi[idx, 0], pi[idx, 1], pi[idx, 2])    # :476
        blocked[idx[hit]] = True
        live[idx[hit]] = False
        idx = idx[~hit]
        p = pos[idx]
        ray = (add[idx] + sign[idx] * (p - pi[idx].astype(F))) / ln[idx]
        speed = ray[:, 0]                                                   # std::min({a, b, c})
        speed = np.where(ray[:, 1] < speed, ray[:, 1], speed)
        speed = np.where(ray[:, 2] < speed, ray[:, 2], speed)
        speed = speed + F(0.002)                                            # :482
        dist[idx] = dist[idx] + speed
        p = p + d[idx] * speed[:, None]
        assert p.dtype == F and speed.dtype == F
        pos[idx] = p
        pi[idx] = to_i32(p)
        i[idx] += 1
    return ~blocked & (dist >= max_dist)                                    # :490


def render(scene, width, height, textures, dyn_textures, colors, shade=True):
    """World::UpdateImage over the whole width x height frame.

    Returns a dict: rgba (h, w, 4) uint8 (None without `shade`), depth (h, w) float32, cell, face,
    steps (h, w) int32 as include/sfrt.h defines the planes, bad_texels (reads outside a texture,
    the oracle's count), zero_dir (some ray has a zero direction component) and maxiter."""
    with np.errstate(all="ignore"):
        return _render(scene, int(width), int(height), textures, dyn_textures, colors, shade)


def _render(scene, W, H, textures, dyn_textures, colors, shade):
    blocks = np.asarray(scene.blocks, dtype=np.int16)
    dyn, lights = scene.dyn, scene.lights
    ndyn = dyn.shape[0]
    cam = np.array(scene.cam_pos, dtype=F)
    view, shadow = F(scene.view_distance), F(scene.shadow_distance)
    maxiter = int(to_u32(view * F(1.5)))                                    # :322
    dx, dz, at, dy, ysc = frame_rays(scene, W, H)
    n = W * H
    col = np.tile(np.arange(W), H)
    row = np.repeat(np.arange(H), W)
    d = np.stack([dx[col], dy[row], dz[col]], axis=1)
    yscale, atan_dir = ysc[row], at[col]
    add, sign, ln = _dda_terms(d)
    # per billboard: atan2f of VNormalizeXZ(d->pos - cam.pos) (:361, :282-285)
    if ndyn:
        e = dyn["pos"].astype(F) - cam
        lxz = np.sqrt(e[:, 0] * e[:, 0] + e[:, 2] * e[:, 2])
        dyn_atan = _map("atan2f", e[:, 2] / lxz, e[:, 0] / lxz)
        dyn_dist = dyn["dist_to_camera"].astype(F)
    dist = np.zeros(n, dtype=F)
    pos = np.broadcast_to(cam, (n, 3)).copy()
    try_pos = pos.copy()
    pi = to_i32(pos)
    di = np.zeros(n, dtype=np.int64)
    col_ray = np.zeros(n, dtype=np.int32)
    i = np.zeros(n, dtype=np.int64)
    steps = np.zeros(n, dtype=np.int32)
    face = np.zeros(n, dtype=np.int32)
    cell = np.full(n, -1, dtype=np.int32)
    depth = np.zeros(n, dtype=F)
    rgba = np.zeros((n, 4), dtype=np.uint8)
    rgba[:, 3] = 255                                                        # sf::Color::Black
    hit_id = np.zeros(n, dtype=np.int16)
    bad_texels = 0
    live = np.ones(n, dtype=bool)
    while True:
        out = live & ~((dist < view) & (i < maxiter))                       # :324
        depth[out] = dist[out]
        live &= ~out
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        steps[idx] += 1
        p = pos[idx]
        ray = (add[idx] + sign[idx] * (p - pi[idx].astype(F))) / ln[idx]
        xr, yr, zr = ray[:, 0], ray[:, 1], ray[:, 2]
        c1 = (xr <= yr) & (xr <= zr)                                        # :329
        c2 = ~c1 & (yr <= xr) & (yr <= zr)                                  # :336
        speed = np.where(c1, xr, np.where(c2, yr, zr))
        speed2 = speed + F(0.002)
        move = np.stack([np.where(c1, speed2, speed), np.where(c2, speed2, speed),
                         np.where(c1 | c2, speed, speed2)], axis=1)
        tp = try_pos[idx] + d[idx] * move
        assert tp.dtype == F and speed.dtype == F
        try_pos[idx] = tp
        col_ray[idx] = np.where(c1, 1, np.where(c2, 2, 3))
        try_dist = dist[idx] + speed                                        # :351
        # dynamic billboards before the next block, :353-378
        returned = np.zeros(idx.size, dtype=bool)
        while ndyn:
            k = di[idx]
            m = ~returned & (k < ndyn)
            mm = np.flatnonzero(m)
            m[mm] = try_dist[mm] >= dyn_dist[k[mm]]
            if not m.any():
                break
            for kk in np.unique(k[m]):
                g = np.flatnonzero(m & (k == kk))
                r = idx[g]
                dd = dyn[kk]
                sp = dyn_dist[kk] - dist[r]
                dist[r] = dyn_dist[kk]
                pp = pos[r] + d[r] * sp[:, None]
                pos[r] = pp
                to = F(dd["pos"][1]) - pp[:, 1]
                sizey = F(dd["size"][1]) * yscale[r]
                inside = np.abs(to) < sizey
                ang = dyn_atan[kk] - atan_dir[r]                            # VAngleXZ, :271-275
                ang = np.where(ang > PI, ang - PI2, np.where(ang < -PI, ang + PI2, ang))
                ang = ang * dist[r]
                tex = _slot(dyn_textures, int(dd["texture_id"]))
                tw, th = _tex_dims(tex)
                xf = F(0.5) + ang / PI * F(0.5) / F(dd["size"][0])
                inside &= (xf > 0) & (xf < 1)
                tx = to_i32(xf * tw)
                ty = to_i32((sizey + to) / sizey / F(2) * th)
                tx = np.where(tx < 0, 0, tx).astype(np.int64)
                ty = np.where(ty < 0, 0, ty).astype(np.int64)
                assert xf.dtype == F and ang.dtype == F and sizey.dtype == F
                s = np.flatnonzero(inside)
                c, bad = _texel(tex, tx[s], ty[s])
                bad_texels += int(bad.sum())
                opaque = c[:, 3] > 127
                so, co, ro = s[opaque], c[opaque], r[s[opaque]]
                tint = np.array([dd["r"], dd["g"], dd["b"]], dtype=F)
                rgba[ro, :3] = to_u8(_min255(co[:, :3].astype(F) * tint))   # :373
                rgba[ro, 3] = co[:, 3]
                face[ro], cell[ro], depth[ro] = 4, kk, dist[ro]
                returned[g[so]] = True
                live[ro] = False
                keep = np.ones(g.size, dtype=bool)
                keep[so] = False
                di[r[keep]] += 1
        go = ~returned
        r = idx[go]
        dist[r] = try_dist[go]                                              # :380
        pos[r] = try_pos[r]
        pi[r] = to_i32(pos[r])
        hit, ids, key = block_at(blocks, pi[r, 0], pi[r, 1], pi[r, 2])      # :385
        rh = r[hit]
        hit_id[rh] = ids[hit]
        cell[rh] = key[hit].astype(np.int32)
        axis = col_ray[rh]
        face[rh] = axis * sign[rh, axis - 1].astype(np.int32)
        depth[rh] = dist[rh]
        live[rh] = False
        i[r[~hit]] += 1
    # the hit blocks' colour, :386-450 (the light loop only with `shade`)
    rh = np.flatnonzero((face != 0) & (face != 4))
    p, ipos, axis = pos[rh].copy(), pi[rh], col_ray[rh]
    sg = sign[rh].copy()
    c = np.zeros((rh.size, 4), dtype=np.uint8)
    ids = hit_id[rh]
    for bid in np.unique(ids):
        g = np.flatnonzero(ids == bid)
        if bid < 0:
            c[g] = np.asarray(colors, dtype=np.uint8)[-int(bid)]
            continue
        tex = _slot(textures, int(bid))
        tw, th = _tex_dims(tex)
        fr = p[g] - ipos[g].astype(F)
        a = axis[g]
        u = np.where(a == 1, fr[:, 2], fr[:, 0])                            # :395-412
        v = np.where(a == 2, fr[:, 2], fr[:, 1])
        c[g], bad = _texel(tex, to_u32(tw * u), to_u32(th * v))
        bad_texels += int(bad.sum())
        for ax in (1, 2, 3):                                                # get it off the wall
            ga = g[a == ax]
            p[ga, ax - 1] = p[ga, ax - 1] + sg[ga, ax - 1] * F(0.01)
            for other in (0, 1, 2):
                if other != ax - 1:
                    sg[ga, other] = F(0)
    assert p.dtype == F and sg.dtype == F
    if shade:
        hd = depth[rh]
        l0 = F(0.05) / hd - hd * F(0.0001)                                  # :414
        lit = np.where(l0 < F(0), F(0), l0)
        lit = np.stack([lit, lit, lit], axis=1)
        for L in lights:                                                    # :418
            lp = L["pos"].astype(F)
            e = p - lp
            dd = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]  # VLengthS
            addl = F(L["intensity"]) / dd - dd * F(0.002)
            s = np.flatnonzero(addl > 0)
            if s.size == 0:
                continue
            nd = lp - p[s]
            addl = addl[s] * ((nd[:, 0] * sg[s, 0] + nd[:, 1] * sg[s, 1] + nd[:, 2] * sg[s, 2])
                              * F(0.7) + F(0.3))
            pos_add = addl > 0
            s, nd, addl = s[pos_add], nd[pos_add], addl[pos_add]
            free = np.ones(s.size, dtype=bool)
            if int(L["shadows"]):
                sh = np.flatnonzero(hd[s] < shadow)                         # :425
                ndn = nd[sh]
                ll = np.sqrt(ndn[:, 0] * ndn[:, 0] + ndn[:, 1] * ndn[:, 1] + ndn[:, 2] * ndn[:, 2])
                free[sh] = _lraycast(blocks, p[s[sh]], ndn / ll[:, None], ll)
            s, addl = s[free], addl[free]
            assert addl.dtype == F
            lit[s] = lit[s] + addl[:, None] * np.array([L["r"], L["g"], L["b"]], dtype=F)
        rgba[rh, :3] = to_u8(_min255(c[:, :3].astype(F) * lit))             # :446
        rgba[rh, 3] = c[:, 3]
    assert depth.dtype == F and dist.dtype == F
    zero_dir = bool((d == 0).any())
    return {"rgba": rgba.reshape(H, W, 4) if shade else None,
            "depth": depth.reshape(H, W), "cell": cell.reshape(H, W), "face": face.reshape(H, W),
            "steps": steps.reshape(H, W), "bad_texels": bad_texels, "zero_dir": zero_dir,
            "maxiter": maxiter}


PLANES = ("depth", "cell", "face", "steps")


def first_sample(ref, s):
    """The planes of each output pixel's first sample, (S*i, S*j), of an S-times larger frame."""
    return {k: ref[k][::s, ::s] for k in PLANES}


def box_filter(rgba, s):
    """SFRT_OPT_SUPERSAMPLE's filter: per byte (sum of the S*S samples + S*S/2) >> log2(S*S)."""
    h, w = rgba.shape[0] // s, rgba.shape[1] // s
    t = rgba.reshape(h, s, w, s, 4).astype(np.uint32).sum(axis=(1, 3))
    return ((t + s * s // 2) // (s * s)).astype(np.uint8)
