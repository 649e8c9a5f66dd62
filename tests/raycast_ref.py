"""SphereWorld::Raycast for arbitrary rays, restated in numpy binary32 (test helper).

The oracle (oracle/sphereworld_oracle.c) answers only the pixels of a pinhole frame.  This
module restates, for whole batches of rays at once,

  * the ray setup of SphereWorld::UpdateImage (SphereWorld.cpp:85-106, with VRotateX /
    VRotateY of :27-36): `pixel_dirs`, the un-normalised direction Raycast receives for
    pixel (i, j);
  * SphereWorld::Raycast (SphereWorld.cpp:355-382) with cam.pos replaced by a per-ray origin:
    `raycast`.

Every operation is a float32 numpy operation in the reference's operand order (numpy neither
contracts nor reassociates; + - * / and sqrt are correctly rounded); sinf / cosf / atan2f / asinf
are the host libm's through ctypes, the functions the reference calls.  The restatement is
trusted only because tests/test_cast_rays.py pins it to the oracle: for the frame's own rays it
must reproduce Oracle.dump and Oracle.render bit for bit.

An invalid ray (include/sfrt.h: a non-finite direction or origin component, or
s = (dx*dx + dy*dy) + dz*dz not a finite normal number) is never marched: sphere -1, zeros
elsewhere.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
PI = F(3.1415926535)     # SphereWorld.h:6
PI2 = F(6.28318530718)   # SphereWorld.h:7

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name, _n in (("sinf", 1), ("cosf", 1), ("asinf", 1), ("atan2f", 2)):
    _fn = getattr(_libm, _name)
    _fn.argtypes = [ctypes.c_float] * _n
    _fn.restype = ctypes.c_float


def _map(name, *args):
    fn = getattr(_libm, name)
    arrs = np.broadcast_arrays(*[np.asarray(a, dtype=F) for a in args])
    out = np.fromiter((fn(*(float(v) for v in vs)) for vs in zip(*(a.ravel() for a in arrs))),
                      dtype=F, count=arrs[0].size)
    return out.reshape(arrs[0].shape)


def _rot_x(v, amount):
    """VRotateX, SphereWorld.cpp:27-31."""
    s, c = F(_libm.sinf(float(amount))), F(_libm.cosf(float(amount)))
    x, y, z = (F(t) for t in v)
    return (x, F(F(y * c) - F(z * s)), F(F(y * s) + F(z * c)))


def _rot_y(v, amount):
    """VRotateY, SphereWorld.cpp:32-36."""
    s, c = F(_libm.sinf(float(amount))), F(_libm.cosf(float(amount)))
    x, y, z = (F(t) for t in v)
    return (F(F(x * c) + F(z * s)), y, F(F(F(-x) * s) + F(z * c)))


def pixel_dirs(scene, width, height):
    """(height, width, 3) float32: r->dir of pixel (i, j) as SphereWorld.cpp:106 builds it."""
    fov_h, fov_v = F(scene.fov_h), F(scene.fov_v)
    rot, hrot = F(scene.rotation), F(scene.hrotation)
    v_start = F(-fov_v)                          # :85
    v_inc = F(F(fov_v / F(height)) * F(2))       # :86
    h_start = F(-fov_h)                          # :88
    h_inc = F(F(fov_h / F(width)) * F(2))        # :89
    up = _rot_x((0, -1, 0), F(-hrot))            # :100
    forward = _rot_x((0, 0, 1), F(-hrot))        # :101
    right = _rot_y((1, 0, 0), rot)               # :102
    forward = _rot_y(forward, rot)               # :103
    up = _rot_y(up, rot)                         # :104
    i = np.arange(width, dtype=F)[None, :]
    j = np.arange(height, dtype=F)[:, None]
    hray = h_start + h_inc * i                   # :95
    vray = v_start + j * v_inc                   # :98
    out = np.empty((height, width, 3), dtype=F)
    for c in range(3):                           # :106
        out[..., c] = (forward[c] + right[c] * hray) + up[c] * vray
    assert out.dtype == F and hray.dtype == F and vray.dtype == F
    return out


def _vlength(x, y, z):
    """VLength, SphereWorld.cpp:340-343."""
    return np.sqrt((x * x + y * y) + z * z)


def raycast(spheres, cam_pos, dirs, origins=None, textures=None, sphere_tex=None,
            max_steps=100000):
    """Raycast (SphereWorld.cpp:355-382) for every ray of `dirs` ((N, 3) float32, un-normalised).

    origins: (N, 3) float32, or None for cam_pos.  textures: {slot: (rgba bytes, w, h)} with
    slot 0 = textures[0], sphere_tex: slot per sphere (None: 0) -- needed for "rgba" only.
    Returns a dict: pos (N, 3), depth (N,), sphere (N,), steps (N,), valid (N,) and, with
    textures, rgba (N, 4) uint8 plus inside (N,): the texel index lay inside the texture."""
    sph = np.asarray(spheres, dtype=F).reshape(-1, 4)
    d = np.ascontiguousarray(np.asarray(dirs, dtype=F).reshape(-1, 3))
    n = d.shape[0]
    if origins is None:
        o = np.broadcast_to(np.asarray(cam_pos, dtype=F), (n, 3)).copy()
    else:
        o = np.ascontiguousarray(np.asarray(origins, dtype=F).reshape(-1, 3))
    with np.errstate(all="ignore"):
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        valid = (np.isfinite(d).all(axis=1) & np.isfinite(o).all(axis=1) & np.isfinite(s) &
                 (s >= np.finfo(F).tiny))
        v = np.flatnonzero(valid)
        pos = o[v].copy()                                     # :357
        length = np.sqrt(s[v])
        dn = d[v] / length[:, None]                           # :358
    assert dn.dtype == F and pos.dtype == F
    draw = np.zeros(v.size, dtype=np.int32)                   # :360
    steps = np.zeros(v.size, dtype=np.int32)
    live = np.ones(v.size, dtype=bool)                        # largestDist = 1 (:359)
    while live.any():                                         # :362
        idx = np.flatnonzero(live)
        p = pos[idx]
        largest = np.zeros(idx.size, dtype=F)                 # :363
        dr = draw[idx]
        for k in range(sph.shape[0]):                         # :364
            dist = _vlength(p[:, 0] - sph[k, 0], p[:, 1] - sph[k, 1], p[:, 2] - sph[k, 2])
            t = sph[k, 3] - dist
            hit = t > F(0.01)                                 # :366
            largest = np.where(hit, np.maximum(largest, t), largest)  # :367
            dr = np.where(hit, np.int32(k), dr)               # :368
        assert largest.dtype == F
        pos[idx] = p + dn[idx] * largest[:, None]             # :371
        draw[idx] = dr
        steps[idx] += 1
        live[idx] = largest > 0
        if int(steps.max(initial=0)) > max_steps:
            raise RuntimeError("raycast_ref: a ray did not end")
    e = pos - o[v]
    depth = _vlength(e[:, 0], e[:, 1], e[:, 2])               # :375's VLength
    out = {"valid": valid,
           "pos": np.zeros((n, 3), dtype=F), "depth": np.zeros(n, dtype=F),
           "sphere": np.full(n, -1, dtype=np.int32), "steps": np.zeros(n, dtype=np.int32)}
    out["pos"][v] = pos
    out["depth"][v] = depth
    out["sphere"][v] = draw
    out["steps"][v] = steps
    if textures is not None:
        c = sph[draw]
        # VAngleXZ(r->pos, centre), :324-328 and :373
        ang = _map("atan2f", c[:, 2], c[:, 0]) - _map("atan2f", pos[:, 2], pos[:, 0])
        ang = np.where(ang > PI, ang - PI2, np.where(ang < -PI, ang + PI2, ang))
        xcoord = ang / PI2 + F(1.0)
        q = pos - c[:, :3]
        ny = q[:, 1] / _vlength(q[:, 0], q[:, 1], q[:, 2])    # VNormalize(..).y, :374
        ycoord = _map("asinf", ny) / PI + F(0.5)
        brightness = F(3.0) / np.maximum(depth, F(3.0))       # :375
        slot = np.zeros(v.size, dtype=np.int64) if sphere_tex is None else \
            np.asarray(sphere_tex, dtype=np.int64)[draw]
        tw = np.array([textures[int(k)][1] for k in slot], dtype=np.int64)
        th = np.array([textures[int(k)][2] for k in slot], dtype=np.int64)
        fu = xcoord * F(4) * c[:, 3]
        fw = ycoord * F(2) * c[:, 3]
        assert fu.dtype == F and fw.dtype == F and brightness.dtype == F
        # fmodf(v, 1.0f) == v - truncf(v) exactly; (unsigned)(float) as x86-64's cvttss2si
        fx = (fu - np.trunc(fu)) * tw.astype(F)
        fy = (fw - np.trunc(fw)) * th.astype(F)
        tx = fx.astype(np.int64) & 0xffffffff
        ty = fy.astype(np.int64) & 0xffffffff
        ti = (tx + ty * tw) & 0xffffffff
        inside = ti < tw * th
        rgba = np.zeros((v.size, 4), dtype=np.uint8)
        for k in np.unique(slot):
            m = (slot == k) & inside
            tex = np.asarray(textures[int(k)][0], dtype=np.uint8).reshape(-1, 4)
            px = tex[ti[m]]
            for ch in range(3):                               # :378-380
                rgba[m, ch] = (px[:, ch].astype(F) * brightness[m]).astype(np.int32).astype(np.uint8)
            rgba[m, 3] = px[:, 3]
        out["rgba"] = np.zeros((n, 4), dtype=np.uint8)
        out["rgba"][v] = rgba
        out["inside"] = np.ones(n, dtype=bool)
        out["inside"][v] = inside
    return out
