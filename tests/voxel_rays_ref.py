"""World::Raycast / World::LRaycast for caller-supplied rays, restated in numpy binary32 (test
helper): the reference of sfrt_voxel_cast_rays and sfrt_voxel_cast_shadow_rays (include/sfrt.h).

`raycast` is voxel_ref.render's march (World.cpp:302-453) with the ray setup of UpdateImage taken
out: each ray brings its own direction (r->dir verbatim), r->yscale and, optionally, its own origin
in cam.pos's place -- then without the billboard loop, as the header defines it.  It keeps what
ended each ray (depth, cell, face, steps as voxel_ref defines the planes) and r->pos at that point.
The conversions, the block lookup, the texel rule and the shadow march are voxel_ref's (to_i32,
to_u32, to_u8, block_at, _texel, _lraycast): nothing of them is written again here, and
tests/test_voxel_cast_rays.py pins this march to voxel_ref.render and to the oracle's frame on the
frame's own rays.

`lraycast` is voxel_ref._lraycast with the trip count the header calls `steps`: the number of
times the body of the `for` at :475 is entered.  No oracle stands behind that count: this
restatement defines it (its booleans are pinned to voxel_ref._lraycast on the colour path's own
shadow rays).

Invalid rays (sfrt.h) are decided here as there, before the march, and get the defined answers.
"""
import numpy as np

import voxel_ref
from voxel_ref import (F, PI, PI2, _dda_terms, _map, _min255, _slot, _tex_dims, _texel, block_at,
                       to_i32, to_u32, to_u8)

MAX_SHADOW_DIST = F(4096.0)   # SFRT_VOXEL_MAX_SHADOW_DIST
OUTPUTS = ("pos", "depth", "cell", "face", "steps", "rgba")


def frame_ray_set(scene, width, height):
    """The frame's own rays as a batch in row-major pixel order: (dirs (n, 3), yscales (n,))."""
    dx, dz, _, dy, ysc = voxel_ref.frame_rays(scene, width, height)
    col = np.tile(np.arange(width), height)
    row = np.repeat(np.arange(height), width)
    return np.stack([dx[col], dy[row], dz[col]], axis=1).astype(F), ysc[row].astype(F)


def raycast(scene, dirs, yscales, origins, textures, dyn_textures, colors, shade=True):
    """World::Raycast for rays (dirs[q], yscales[q]) from origins[q], or from scene.cam_pos with
    the billboards when origins is None (yscales None: 1.0f).

    Returns a dict: pos (n, 3) float32, depth (n,) float32, cell, face, steps (n,) int32, rgba
    (n, 4) uint8 (None without `shade`), bad_texels (reads outside a texture), maxiter, valid (n,)
    bool.  An invalid ray has face 0, cell -1, steps 0 and zeros elsewhere."""
    d = np.ascontiguousarray(np.asarray(dirs, dtype=F).reshape(-1, 3))
    n = d.shape[0]
    ys = np.ones(n, dtype=F) if yscales is None else np.asarray(yscales, dtype=F).reshape(n)
    own = origins is not None
    org = np.asarray(origins, dtype=F).reshape(n, 3) if own else \
        np.broadcast_to(np.array(scene.cam_pos, dtype=F), (n, 3))
    valid = np.isfinite(d).all(axis=1) & np.isfinite(ys) & np.isfinite(org).all(axis=1)
    v = np.flatnonzero(valid)
    with np.errstate(all="ignore"):
        r = _march(scene, d[v], ys[v], org[v].copy(), own, textures, dyn_textures, colors, shade)
    out = {"pos": np.zeros((n, 3), dtype=F), "depth": np.zeros(n, dtype=F),
           "cell": np.full(n, -1, dtype=np.int32), "face": np.zeros(n, dtype=np.int32),
           "steps": np.zeros(n, dtype=np.int32),
           "rgba": np.zeros((n, 4), dtype=np.uint8) if shade else None}
    for k in OUTPUTS:
        if out[k] is not None:
            out[k][v] = r[k]
    out.update(bad_texels=r["bad_texels"], maxiter=r["maxiter"], valid=valid)
    return out


def _march(scene, d, yscale, org, own, textures, dyn_textures, colors, shade):
    blocks = np.asarray(scene.blocks, dtype=np.int16)
    dyn, lights = scene.dyn, scene.lights
    ndyn = 0 if own else dyn.shape[0]                                       # own origins: no billboards
    cam = np.array(scene.cam_pos, dtype=F)
    view, shadow = F(scene.view_distance), F(scene.shadow_distance)
    maxiter = int(to_u32(view * F(1.5)))                                    # :322
    n = d.shape[0]
    add, sign, ln = _dda_terms(d)
    if ndyn:
        atan_dir = _map("atan2f", d[:, 2], d[:, 0])                         # VAngleXZ's ray term, :272
        e = dyn["pos"].astype(F) - cam
        lxz = np.sqrt(e[:, 0] * e[:, 0] + e[:, 2] * e[:, 2])
        dyn_atan = _map("atan2f", e[:, 2] / lxz, e[:, 0] / lxz)
        dyn_dist = dyn["dist_to_camera"].astype(F)
    dist = np.zeros(n, dtype=F)
    pos = org.copy()                                                        # :305
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
        returned = np.zeros(idx.size, dtype=bool)
        while ndyn:                                                         # :353-378
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
                pos[r] = pp                                                 # :357
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
        pos[r] = try_pos[r]                                                 # :381
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
    end_pos = pos.copy()  # r->pos where Raycast ended: :381 (before :396-408), :357, or the loop's exit
    if shade:
        bad_texels += _shade(blocks, lights, shadow, textures, colors, pos, pi, col_ray, sign, hit_id,
                             face, depth, rgba)
    assert depth.dtype == F and dist.dtype == F and end_pos.dtype == F
    return {"pos": end_pos, "depth": depth, "cell": cell, "face": face, "steps": steps,
            "rgba": rgba if shade else None, "bad_texels": bad_texels, "maxiter": maxiter}


def _shade(blocks, lights, shadow, textures, colors, pos, pi, col_ray, sign, hit_id, face, depth, rgba):
    """The hit blocks' colour, :386-450, into rgba; returns the texel reads outside a texture."""
    bad_texels = 0
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
    hd = depth[rh]
    l0 = F(0.05) / hd - hd * F(0.0001)                                      # :414
    lit = np.where(l0 < F(0), F(0), l0)
    lit = np.stack([lit, lit, lit], axis=1)
    for L in lights:                                                        # :418
        lp = L["pos"].astype(F)
        e = p - lp
        dd = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]      # VLengthS
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
            sh = np.flatnonzero(hd[s] < shadow)                             # :425
            ndn = nd[sh]
            ll = np.sqrt(ndn[:, 0] * ndn[:, 0] + ndn[:, 1] * ndn[:, 1] + ndn[:, 2] * ndn[:, 2])
            free[sh] = voxel_ref._lraycast(blocks, p[s[sh]], ndn / ll[:, None], ll)
        s, addl = s[free], addl[free]
        assert addl.dtype == F
        lit[s] = lit[s] + addl[:, None] * np.array([L["r"], L["g"], L["b"]], dtype=F)
    rgba[rh, :3] = to_u8(_min255(c[:, :3].astype(F) * lit))                 # :446
    rgba[rh, 3] = c[:, 3]
    return bad_texels


def lraycast(blocks, pos, d, max_dist):
    """World::LRaycast, World.cpp:455-491, for n valid rays: (free (n,) bool, steps (n,) int32).
    The march is voxel_ref._lraycast's, statement for statement, plus the count of the trips of
    the loop's body (the one that returns false included), which this restatement defines."""
    blocks = np.asarray(blocks, dtype=np.int16)
    n = pos.shape[0]
    pos = np.asarray(pos, dtype=F).copy()
    d = np.asarray(d, dtype=F)
    max_dist = np.asarray(max_dist, dtype=F)
    dist = np.zeros(n, dtype=F)
    pi = to_i32(pos)
    add, sign, ln = _dda_terms(d)
    m2 = max_dist * F(2)
    max_iter = to_u32(np.where(m2 < F(20.0), F(20.0), m2))                 # :473
    blocked = np.zeros(n, dtype=bool)
    i = np.zeros(n, dtype=np.int64)
    steps = np.zeros(n, dtype=np.int32)
    live = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        while True:
            live &= (i < max_iter) & (dist < max_dist)                      # :475
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            steps[idx] += 1
            hit, _, _ = block_at(blocks, pi[idx, 0], pi[idx, 1], pi[idx, 2])    # :476
            blocked[idx[hit]] = True
            live[idx[hit]] = False
            idx = idx[~hit]
            p = pos[idx]
            ray = (add[idx] + sign[idx] * (p - pi[idx].astype(F))) / ln[idx]
            speed = ray[:, 0]                                               # std::min({a, b, c})
            speed = np.where(ray[:, 1] < speed, ray[:, 1], speed)
            speed = np.where(ray[:, 2] < speed, ray[:, 2], speed)
            speed = speed + F(0.002)                                        # :482
            dist[idx] = dist[idx] + speed
            p = p + d[idx] * speed[:, None]
            assert p.dtype == F and speed.dtype == F
            pos[idx] = p
            pi[idx] = to_i32(p)
            i[idx] += 1
    return ~blocked & (dist >= max_dist), steps                             # :490


def shadow_rays(scene, origins, dirs, max_dists):
    """sfrt_voxel_cast_shadow_rays: {free: 1 / 0 / -1 (invalid), steps} as int32, and `valid`."""
    o = np.asarray(origins, dtype=F).reshape(-1, 3)
    d = np.asarray(dirs, dtype=F).reshape(-1, 3)
    md = np.asarray(max_dists, dtype=F).ravel()
    with np.errstate(all="ignore"):
        valid = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(md) & \
            (md <= MAX_SHADOW_DIST)
    v = np.flatnonzero(valid)
    free = np.full(md.shape[0], -1, dtype=np.int32)
    steps = np.zeros(md.shape[0], dtype=np.int32)
    f, s = lraycast(scene.blocks, o[v], d[v], md[v])
    free[v] = f.astype(np.int32)
    steps[v] = s
    return {"free": free, "steps": steps, "valid": valid}
