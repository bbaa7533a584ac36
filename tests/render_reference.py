"""An fp64 numpy ray caster for the render tests, written from the description in include/ppenv_render.h and independent of
isaacgym_amd/csrc/ppenv_render_device.h (textbook quadratic forms, vectorised over rays), plus the decided / edge rule.
TEST INFRASTRUCTURE ONLY.

A pixel is DECIDED when casting its ray at the eight offsets of +-1/8 pixel in x and / or y gives the same primitive id, shadow flag and
checker parity as its centre, and a depth within 2 % of the centre's (a depth that moves faster than that under an eighth of a pixel is
a grazing hit, where fp32 rounding of the discriminant is amplified without bound).  Every other pixel is an EDGE pixel."""
import numpy as np

T_MIN, SHADOW_OFFSET = 1e-4, 1e-3
SPHERE, CAPSULE, BOX, CYLINDER, BONE = range(5)
SKY, GROUND = -1, -2


def quat_rotate(q, v):
    """my_quat_rotate (xyzw), the formula the pose tensors' consumers use: v (2w^2 - 1) + 2w (qv x v) + 2 qv (qv . v)."""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    qv, w = q[:3], q[3]
    return v * (2 * w * w - 1) + 2 * w * np.cross(qv, v) + 2 * qv * np.dot(qv, v)


def place(prims, sources, env):
    """prims: Scene.prims dicts; sources: [array [N, rows, 13]] -> list of posed dicts (kind, a, b, radius, axes [3, 3], albedo) in fp64."""
    out = []
    for p in prims:
        a, b, kind, axes = np.asarray(p["a"], np.float64), np.asarray(p["b"], np.float64), p["kind"], np.eye(3)
        if kind == BONE:
            src = np.asarray(sources[p["source"]], np.float64)
            a, b, kind = src[env, p["row"], :3], src[env, p["row2"], :3], CAPSULE
        elif p["row"] >= 0:
            s = np.asarray(sources[p["source"]], np.float64)[env, p["row"]]
            a = s[:3] + quat_rotate(s[3:7], a)
            if kind == BOX:
                axes = np.stack([quat_rotate(s[3:7], e) for e in np.eye(3)])
            else:
                b = s[:3] + quat_rotate(s[3:7], b)
        out.append(dict(kind=kind, a=a, b=b, radius=float(p["radius"]), axes=axes, albedo=np.asarray(p["albedo"], np.float64)))
    return out


def posed_matrix(posed):
    """The posed dicts in pp_render_posed's 20-word layout: a, radius, b, kind (NOT comparable as a float: column 7), axes, albedo."""
    return np.array([np.concatenate([p["a"], [p["radius"]], p["b"], [p["kind"]], p["axes"].reshape(-1), p["albedo"]]) for p in posed])


def _sphere(c, r, o, d):
    oc = o - c
    b = oc @ d.T if oc.ndim == 1 else np.einsum("ij,ij->i", oc, d)
    cc = np.sum(oc * oc, axis=-1) - r * r
    disc = b * b - cc
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    ok = (disc >= 0) & (t > T_MIN)
    t = np.where(ok, t, np.inf)
    oc = np.broadcast_to(oc, d.shape)
    with np.errstate(invalid="ignore"):
        n = (oc + d * np.where(ok, t, 0.0)[:, None]) / r
    return t, n


def _rod(a, b, r, flat, o, d):
    ba = b - a
    ln = np.linalg.norm(ba)
    if ln * ln <= 1e-12:
        return (np.full(len(d), np.inf), np.zeros_like(d)) if flat else _sphere(a, r, o, d)
    u = ba / ln
    oa = np.broadcast_to(o - a, d.shape)
    ou, du = oa @ u, d @ u
    op, dp = oa - ou[:, None] * u, d - du[:, None] * u
    A, B, Cc = np.sum(dp * dp, -1), np.sum(op * dp, -1), np.sum(op * op, -1) - r * r
    with np.errstate(invalid="ignore", divide="ignore"):
        disc = B * B - A * Cc
        t = (-B - np.sqrt(disc)) / A
        y = ou + t * du
        ok = (A > 1e-12) & (disc >= 0) & (t > T_MIN) & (y >= 0) & (y <= ln)
    best = np.where(ok, t, np.inf)
    n = np.where(ok[:, None], (op + dp * np.where(ok, t, 0.0)[:, None]) / r, 0.0)
    if flat:
        with np.errstate(invalid="ignore", divide="ignore"):
            y0 = np.where(du > 0, 0.0, ln)
            tc = (y0 - ou) / du
            w = op + dp * np.where(np.isfinite(tc), tc, 0.0)[:, None]
            okc = (du != 0) & (tc > T_MIN) & (tc < best) & (np.sum(w * w, -1) <= r * r)
        best = np.where(okc, tc, best)
        n = np.where(okc[:, None], np.where(du > 0, -1.0, 1.0)[:, None] * u, n)
    else:
        for c, sgn in ((a, -1.0), (b, 1.0)):
            ts, ns = _sphere(c, r, o, d)
            okc = (ts < best) & (sgn * (ns @ u) >= 0)
            best = np.where(okc, ts, best)
            n = np.where(okc[:, None], ns, n)
    return best, n


def _box(c, half, axes, o, d):
    oc = np.broadcast_to(o - c, d.shape)
    tn, tf = np.full(len(d), -np.inf), np.full(len(d), np.inf)
    n = np.zeros_like(d)
    miss = np.zeros(len(d), bool)
    for k in range(3):
        ol, dl = oc @ axes[k], d @ axes[k]
        par = dl == 0
        miss |= par & ((ol < -half[k]) | (ol > half[k]))
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (-half[k] - ol) / dl, (half[k] - ol) / dl
        lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
        upd = ~par & (lo > tn)
        tn = np.where(upd, lo, tn)
        n = np.where(upd[:, None], np.where(dl > 0, -1.0, 1.0)[:, None] * axes[k], n)
        tf = np.where(~par & (hi < tf), hi, tf)
    ok = ~miss & (tn <= tf) & (tn > T_MIN)
    return np.where(ok, tn, np.inf), n


def _hit(p, o, d):
    if p["kind"] == SPHERE:
        return _sphere(p["a"], p["radius"], o, d)
    if p["kind"] in (CAPSULE, CYLINDER):
        return _rod(p["a"], p["b"], p["radius"], p["kind"] == CYLINDER, o, d)
    if p["kind"] == BOX:
        return _box(p["a"], p["b"], p["axes"], o, d)
    return np.full(len(d), np.inf), np.zeros_like(d)


def basis(eye, target, up):
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    return f, r, np.cross(r, f)


def project(point, eye, target, up, fov_deg, width, height):
    """World point -> (px, py) in pixel units (the centre of pixel (x, y) is (x + 0.5, y + 0.5))."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f, r, u = basis(eye, target, up)
    v = np.asarray(point, np.float64) - eye
    th = np.tan(np.radians(fov_deg) / 2)
    s, t = (v @ r) / (v @ f), (v @ u) / (v @ f)
    return (s / (th * width / height) + 1) * width / 2, (1 - t / th) * height / 2


def cast(posed, header, eye, target, up, fov_deg, width, height, dx=0.0, dy=0.0):
    """One ray per pixel through (x + 0.5 + dx, y + 0.5 + dy).  header: dict(ground_z, checker, checker_pitch, ground_rgb, sky_rgb, light,
    ambient, diffuse).  -> dict(id, depth, shadow, parity [H, W], rgb [H, W, 3] float in [0, 1])."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f, r, u = basis(eye, target, up)
    th = np.tan(np.radians(fov_deg) / 2)
    ys, xs = np.mgrid[0:height, 0:width]
    px, py = xs.reshape(-1) + 0.5 + dx, ys.reshape(-1) + 0.5 + dy
    s = (2 * px / width - 1) * th * width / height
    t = (1 - 2 * py / height) * th
    d = f + s[:, None] * r + t[:, None] * u
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R = len(d)
    depth, ids, n = np.full(R, np.inf), np.full(R, SKY), np.tile([0.0, 0.0, 1.0], (R, 1))
    for i, p in enumerate(posed):
        ti, ni = _hit(p, eye, d)
        upd = ti < depth
        depth, ids, n = np.where(upd, ti, depth), np.where(upd, i, ids), np.where(upd[:, None], ni, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = (header["ground_z"] - eye[2]) / d[:, 2]
    upd = (d[:, 2] < 0) & (tg > T_MIN) & (tg < depth)
    depth, ids, n = np.where(upd, tg, depth), np.where(upd, GROUND, ids), np.where(upd[:, None], [0.0, 0.0, 1.0], n)
    hit = ids != SKY
    pt = eye + d * np.where(hit, depth, 0.0)[:, None]
    parity = np.zeros(R, int)
    if header["checker"]:
        par = (np.floor(pt[:, 0] / header["checker_pitch"]) + np.floor(pt[:, 1] / header["checker_pitch"])).astype(np.int64) & 1
        parity = np.where(ids == GROUND, par, 0)
    albedo = np.asarray(header["ground_rgb"], np.float64)[parity]
    for i, p in enumerate(posed):
        albedo = np.where((ids == i)[:, None], p["albedo"], albedo)
    light = np.asarray(header["light"], np.float64)
    ndl = n @ light
    shadow = np.zeros(R, bool)
    so = pt + n * SHADOW_OFFSET
    lit = hit & (ndl > 0)
    if lit.any():
        sub = np.flatnonzero(lit)
        blocked = np.zeros(len(sub), bool)
        dl = np.tile(light, (len(sub), 1))
        for p in posed:
            ts, _ = _hit(p, so[sub], dl)
            blocked |= np.isfinite(ts)
        shadow[sub] = blocked
    rgb = albedo * (header["ambient"] + header["diffuse"] * np.where(lit & ~shadow, ndl, 0.0))[:, None]
    rgb = np.where(hit[:, None], rgb, np.asarray(header["sky_rgb"], np.float64))
    sh = (height, width)
    return dict(id=ids.reshape(sh), depth=depth.reshape(sh), shadow=shadow.reshape(sh).astype(int), parity=parity.reshape(sh), rgb=rgb.reshape(sh + (3,)))


def decided(posed, header, eye, target, up, fov_deg, width, height, centre=None):
    """-> (centre cast, bool [H, W]: the decided pixels)."""
    c = centre if centre is not None else cast(posed, header, eye, target, up, fov_deg, width, height)
    ok = np.ones((height, width), bool)
    for dx in (-0.125, 0.0, 0.125):
        for dy in (-0.125, 0.0, 0.125):
            if dx == 0.0 and dy == 0.0:
                continue
            o = cast(posed, header, eye, target, up, fov_deg, width, height, dx, dy)
            ok &= (o["id"] == c["id"]) & (o["shadow"] == c["shadow"]) & (o["parity"] == c["parity"])
            both = np.isfinite(c["depth"]) & np.isfinite(o["depth"])
            with np.errstate(invalid="ignore"):
                ok &= ~both | (np.abs(o["depth"] - c["depth"]) <= 0.02 * c["depth"])
    return c, ok


def rgb8(rgb):
    """The ABI's channel rule on the fp64 colours."""
    return (255.0 * np.clip(rgb, 0.0, 1.0) + 0.5).astype(np.int64)
