// ppenv_render_device.h — per-primitive and per-pixel arithmetic of the ray caster (include/ppenv_render.h): placing a primitive on its
// body row, the ray of a pixel, the four ray / primitive intersections, the ground, the shading, the RGBA8 packing and the fixed-order box
// mean of a supersampled pixel (render_pixel_aa).
//
// PP_HD like ppenv_play_device.h: the HIP kernels in ppenv_render.hip and the tests' host build (tests/csrc/render_shim.cpp, render_aa_shim.cpp, g++)
// compile this text.  fp32 throughout.  The two builds need not agree bit for bit (sqrtf and the divisions may round differently,
// and the device contracts a * b + c): the tests compare them on the pixels that are not on an edge, DESIGN §5f.
// Depth uses +inf for the sky: this header is compiled without -ffinite-math-only on both sides (isaacgym_amd/_lib.py SOURCE_FLAGS).
#pragma once

#include "ppenv_device.h"
#include "../../include/ppenv_render.h"

namespace pp {

PP_HD float render_inf() { return __builtin_huge_valf(); }

// What the kernels get by value: the camera's orthonormal basis, worked out once on the host.
struct RenderView {
    float eye[3], fwd[3], right[3], up[3];
    float tan_half;                     // tan(fov / 2)
    int32_t width, height, follow_source, follow_row;
};

PP_HD V3 render_normalize(V3 v) { return v * (1.0f / sqrtf(dot(v, v))); }

// fwd = normalize(target - eye), right = normalize(fwd x up), up' = right x fwd
PP_HD void render_view_of(const pp_render_camera& c, RenderView& v) {
    const V3 f = render_normalize(ld3(c.target) - ld3(c.eye));
    const V3 r = render_normalize(cross(f, ld3(c.up)));
    const V3 u = cross(r, f);
    v.eye[0] = c.eye[0]; v.eye[1] = c.eye[1]; v.eye[2] = c.eye[2];
    v.fwd[0] = f.x; v.fwd[1] = f.y; v.fwd[2] = f.z;
    v.right[0] = r.x; v.right[1] = r.y; v.right[2] = r.z;
    v.up[0] = u.x; v.up[1] = u.y; v.up[2] = u.z;
    v.tan_half = tanf(0.5f * c.fov_deg * 0.017453292519943295f);
    v.width = c.width; v.height = c.height;
    v.follow_source = c.follow_source; v.follow_row = c.follow_row;
}

PP_HD const float* render_row(const pp_render_source& s, int32_t env, int32_t row) {
    return s.base + (int64_t)env * s.env_stride + (int64_t)row * s.row_stride;
}

// The follow rule: the body's x and y, not its z.
PP_HD V3 render_follow(const pp_render_scene& sc, const RenderView& v, int32_t env) {
    if (v.follow_row < 0) return mk(0.0f, 0.0f, 0.0f);
    const float* p = render_row(sc.source[v.follow_source], env, v.follow_row);
    return mk(p[0], p[1], 0.0f);
}

// Primitive `pr` of env `env` in world space.
PP_HD void render_place(const pp_render_scene& sc, const pp_render_prim& pr, int32_t env, pp_render_posed& out) {
    V3 a = ld3(pr.a), b = ld3(pr.b);
    V3 ax = mk(1.0f, 0.0f, 0.0f), ay = mk(0.0f, 1.0f, 0.0f), az = mk(0.0f, 0.0f, 1.0f);
    int32_t kind = pr.kind;
    if (kind == PP_RENDER_BONE) {
        a = ld3(render_row(sc.source[pr.source], env, pr.row));
        b = ld3(render_row(sc.source[pr.source], env, pr.row2));
        kind = PP_RENDER_CAPSULE;
    } else if (pr.row >= 0) {
        const float* s = render_row(sc.source[pr.source], env, pr.row);
        const V3 p = ld3(s);
        const float q[4] = {s[3], s[4], s[5], s[6]};
        a = p + quat_rotate(q, a);
        if (kind == PP_RENDER_BOX) {
            ax = quat_rotate(q, ax); ay = quat_rotate(q, ay); az = quat_rotate(q, az);
        } else {
            b = p + quat_rotate(q, b);
        }
    }
    out.a[0] = a.x; out.a[1] = a.y; out.a[2] = a.z;
    out.radius = pr.radius;
    out.b[0] = b.x; out.b[1] = b.y; out.b[2] = b.z;
    out.kind = kind;
    out.axis[0] = ax.x; out.axis[1] = ax.y; out.axis[2] = ax.z;
    out.axis[3] = ay.x; out.axis[4] = ay.y; out.axis[5] = ay.z;
    out.axis[6] = az.x; out.axis[7] = az.y; out.axis[8] = az.z;
    out.albedo[0] = pr.albedo[0]; out.albedo[1] = pr.albedo[1]; out.albedo[2] = pr.albedo[2];
}

PP_HD void render_place_none(pp_render_posed& out) {
    for (int k = 0; k < 3; ++k) out.a[k] = out.b[k] = out.albedo[k] = 0.0f;
    for (int k = 0; k < 9; ++k) out.axis[k] = 0.0f;
    out.radius = 0.0f;
    out.kind = -1;
}

// The ray through the centre of pixel (x, y) — or through (x + 0.5 + dx, y + 0.5 + dy): unit direction.
PP_HD V3 render_ray_dir(const RenderView& v, float px, float py) {
    const float aspect = (float)v.width / (float)v.height;
    const float s = (2.0f * px / (float)v.width - 1.0f) * v.tan_half * aspect;
    const float t = (1.0f - 2.0f * py / (float)v.height) * v.tan_half;
    return render_normalize(ld3(v.fwd) + ld3(v.right) * s + ld3(v.up) * t);
}

// ---- intersections: the nearest t > PP_RENDER_T_MIN at which the ray o + t d (|d| = 1) ENTERS the solid, and the outward normal there.
// A ray that starts inside a solid does not hit it.

// |oc - (oc.d) d|^2 against r^2: no difference of two large squares.
PP_HD bool render_hit_sphere(V3 c, float r, V3 o, V3 d, float& t, V3& n) {
    const V3 oc = o - c;
    const float b = dot(oc, d);
    const V3 l = oc - d * b;
    const float disc = r * r - dot(l, l);
    if (!(disc >= 0.0f)) return false;
    const float tt = -b - sqrtf(disc);
    if (!(tt > PP_RENDER_T_MIN)) return false;
    t = tt;
    n = (oc + d * tt) * (1.0f / r);
    return true;
}

// The side of a cylinder of radius r about the segment a -> a + u * len (u a unit vector), then for a capsule the two end spheres,
// for a capped cylinder the two discs.
PP_HD bool render_hit_rod(V3 a, V3 b, float r, bool flat, V3 o, V3 d, float& t, V3& n) {
    const V3 ba = b - a;
    const float len2 = dot(ba, ba);
    if (!(len2 > 1e-12f)) return flat ? false : render_hit_sphere(a, r, o, d, t, n);
    const float len = sqrtf(len2);
    const V3 u = ba * (1.0f / len);
    const V3 oa = o - a;
    const float ou = dot(oa, u), du = dot(d, u);
    const V3 op = oa - u * ou, dp = d - u * du;          // the parts across the axis
    const float A = dot(dp, dp), B = dot(op, dp);
    bool hit = false;
    float best = render_inf();
    if (A > 1e-12f) {
        const V3 l = op - dp * (B / A);                   // the ray's closest approach to the axis, across it
        const float disc = r * r - dot(l, l);
        if (disc >= 0.0f) {
            const float tt = (-B - sqrtf(disc * A)) / A;
            const float y = ou + tt * du;
            if (tt > PP_RENDER_T_MIN && y >= 0.0f && y <= len) {
                best = tt;
                n = (op + dp * tt) * (1.0f / r);
                hit = true;
            }
        }
    }
    if (flat) {
        if (du != 0.0f) {                                 // the cap the ray meets from outside: a when it runs along +u
            const float y0 = du > 0.0f ? 0.0f : len;
            const float tt = (y0 - ou) / du;
            const V3 w = op + dp * tt;
            if (tt > PP_RENDER_T_MIN && tt < best && dot(w, w) <= r * r) {
                best = tt;
                n = du > 0.0f ? -u : u;
                hit = true;
            }
        }
    } else {
        float tt;
        V3 nn;
        if (render_hit_sphere(a, r, o, d, tt, nn) && tt < best && dot(nn, u) <= 0.0f) { best = tt; n = nn; hit = true; }
        if (render_hit_sphere(b, r, o, d, tt, nn) && tt < best && dot(nn, u) >= 0.0f) { best = tt; n = nn; hit = true; }
    }
    if (hit) t = best;
    return hit;
}

PP_HD bool render_hit_box(const pp_render_posed& p, V3 o, V3 d, float& t, V3& n) {
    const V3 oc = o - ld3(p.a);
    float tn = -render_inf(), tf = render_inf();
    int face = 0;
    float sign = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3 ax = ld3(p.axis + 3 * k);
        const float ol = dot(oc, ax), dl = dot(d, ax), h = p.b[k];
        if (dl == 0.0f) {
            if (ol < -h || ol > h) return false;
            continue;
        }
        const float inv = 1.0f / dl;
        const float t0 = (-h - ol) * inv, t1 = (h - ol) * inv;
        const float lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
        if (lo > tn) { tn = lo; face = k; sign = dl > 0.0f ? -1.0f : 1.0f; }
        if (hi < tf) tf = hi;
    }
    if (!(tn <= tf) || !(tn > PP_RENDER_T_MIN)) return false;
    t = tn;
    n = ld3(p.axis + 3 * face) * sign;
    return true;
}

PP_HD bool render_hit(const pp_render_posed& p, V3 o, V3 d, float& t, V3& n) {
    switch (p.kind) {
    case PP_RENDER_SPHERE: return render_hit_sphere(ld3(p.a), p.radius, o, d, t, n);
    case PP_RENDER_CAPSULE: return render_hit_rod(ld3(p.a), ld3(p.b), p.radius, false, o, d, t, n);
    case PP_RENDER_CYLINDER: return render_hit_rod(ld3(p.a), ld3(p.b), p.radius, true, o, d, t, n);
    case PP_RENDER_BOX: return render_hit_box(p, o, d, t, n);
    default: return false;
    }
}

// Any primitive between `o` and the light?
PP_HD bool render_occluded(const pp_render_posed* posed, int32_t count, V3 o, V3 d) {
    for (int32_t i = 0; i < count; ++i) {
        float t;
        V3 n;
        if (render_hit(posed[i], o, d, t, n)) return true;
    }
    return false;
}

PP_HD uint32_t render_channel(float v) {
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return (uint32_t)(int)(255.0f * c + 0.5f);
}

// little-endian R, G, B, A bytes in one word
PP_HD uint32_t render_pack(V3 c) { return render_channel(c.x) | (render_channel(c.y) << 8) | (render_channel(c.z) << 16) | 0xFF000000u; }

struct RenderPixel {
    uint32_t rgba;
    float depth;
    int32_t id;
    int32_t shadow;                     // 1: the shadow ray was blocked (the tests' fp64 caster reports the same flag)
    int32_t parity;                     // ground hits: the checker cell's parity; otherwise 0
};

// What one ray sees, before the packing: the float colour (not clamped) next to RenderPixel's other fields.
struct RenderSample {
    V3 rgb;
    float depth;
    int32_t id, shadow, parity;
};

// The ray from eye + follow through (px, py) in pixel units (the centre of pixel (x, y) is (x + 0.5, y + 0.5)): primary hit, ground and
// checker, one shadow ray.
PP_HD RenderSample render_sample(const pp_render_scene& sc, const RenderView& v, V3 follow, const pp_render_posed* posed, int32_t count, float px, float py) {
    const V3 o = ld3(v.eye) + follow;
    const V3 d = render_ray_dir(v, px, py);
    RenderSample out;
    out.id = PP_RENDER_ID_SKY;
    out.depth = render_inf();
    out.shadow = 0;
    out.parity = 0;
    V3 n = mk(0.0f, 0.0f, 1.0f);
    for (int32_t i = 0; i < count; ++i) {
        float t;
        V3 ni;
        if (render_hit(posed[i], o, d, t, ni) && t < out.depth) { out.depth = t; out.id = i; n = ni; }
    }
    if (d.z < 0.0f) {
        const float t = (sc.ground_z - o.z) / d.z;
        if (t > PP_RENDER_T_MIN && t < out.depth) { out.depth = t; out.id = PP_RENDER_ID_GROUND; n = mk(0.0f, 0.0f, 1.0f); }
    }
    if (out.id == PP_RENDER_ID_SKY) {
        out.rgb = ld3(sc.sky_rgb);
        return out;
    }
    const V3 p = o + d * out.depth;
    V3 albedo;
    if (out.id == PP_RENDER_ID_GROUND) {
        if (sc.checker) out.parity = ((int32_t)floorf(p.x / sc.checker_pitch) + (int32_t)floorf(p.y / sc.checker_pitch)) & 1;
        albedo = ld3(sc.ground_rgb[out.parity]);
    } else {
        albedo = ld3(posed[out.id].albedo);
    }
    const V3 l = ld3(sc.light);
    const float ndl = dot(n, l);
    float lit = 0.0f;
    if (ndl > 0.0f) {
        out.shadow = render_occluded(posed, count, p + n * PP_RENDER_SHADOW_OFFSET, l) ? 1 : 0;
        lit = out.shadow ? 0.0f : ndl;
    }
    out.rgb = albedo * (sc.ambient + sc.diffuse * lit);
    return out;
}

// One pixel of env `env`: one ray through (px, py), packed.
PP_HD RenderPixel render_pixel(const pp_render_scene& sc, const RenderView& v, V3 follow, const pp_render_posed* posed, int32_t count, float px, float py) {
    const RenderSample s = render_sample(sc, v, follow, posed, count, px, py);
    RenderPixel out;
    out.rgba = render_pack(s.rgb);
    out.depth = s.depth;
    out.id = s.id;
    out.shadow = s.shadow;
    out.parity = s.parity;
    return out;
}

// ---- supersampling: pixel (x, y) is the box mean of s x s rays, s = 1, 2 or 4 sub-samples per axis (pp_render_rays_aa).
constexpr int32_t kRenderMaxSamples = 4;

PP_HD bool render_samples_ok(int32_t s) { return s == 1 || s == 2 || s == 4; }

PP_HD float render_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// Sub-sample k = j * s + i (i, j = 0 .. s - 1) of pixel (x, y): the ray through (x + (i + 1/2) / s, y + (j + 1/2) / s) — exact in fp32, s being a
// power of two — shaded as render_sample does, each channel clamped to [0, 1].
PP_HD V3 render_aa_sample(const pp_render_scene& sc, const RenderView& v, V3 follow, const pp_render_posed* posed, int32_t count, int32_t x, int32_t y,
                          int32_t s, int32_t k) {
    const float inv = 1.0f / (float)s;
    const int32_t i = k % s, j = k / s;
    const V3 c = render_sample(sc, v, follow, posed, count, (float)x + ((float)i + 0.5f) * inv, (float)y + ((float)j + 0.5f) * inv).rgb;
    return mk(render_clamp01(c.x), render_clamp01(c.y), render_clamp01(c.z));
}

// THE ORDER OF THE SUM, per channel: a binary tree over the sub-sample index k.  Level m = 1, 2, 4, 8 (while m < s * s) replaces the value of
// every k that is a multiple of 2m by value[k] + value[k + m]; the total ends in value[0].  The kernel's lanes do the same additions as a
// butterfly (lane k adds the value of lane k ^ m: fp32 addition commutes, so every lane of a pixel holds the bits of value[0]).
PP_HD V3 render_aa_tree_sum(V3* c, int32_t n) {
    for (int32_t m = 1; m < n; m *= 2)
        for (int32_t k = 0; k < n; k += 2 * m) c[k] = c[k] + c[k + m];
    return c[0];
}

// The sum times the exact 1 / s^2, then channel = (int)(255 v + 0.5), alpha 255.
PP_HD uint32_t render_aa_pack(V3 sum, int32_t s) {
    const V3 m = sum * (1.0f / (float)(s * s));
    return (uint32_t)(int)(255.0f * m.x + 0.5f) | ((uint32_t)(int)(255.0f * m.y + 0.5f) << 8) | ((uint32_t)(int)(255.0f * m.z + 0.5f) << 16) | 0xFF000000u;
}

// The supersampled pixel (x, y), sub-sample after sub-sample: what the host build runs and what the kernel's lanes, one per sub-sample, add up to.
PP_HD uint32_t render_pixel_aa(const pp_render_scene& sc, const RenderView& v, V3 follow, const pp_render_posed* posed, int32_t count, int32_t x, int32_t y,
                               int32_t s) {
    V3 c[kRenderMaxSamples * kRenderMaxSamples];
    for (int32_t k = 0; k < s * s; ++k) c[k] = render_aa_sample(sc, v, follow, posed, count, x, y, s, k);
    return render_aa_pack(render_aa_tree_sum(c, s * s), s);
}

}  // namespace pp
