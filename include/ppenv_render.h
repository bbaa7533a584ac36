/*
 * ppenv_render.h — C ABI of the ray caster that draws envs from the state tensors they already expose.
 *
 * A scene is a short list of analytic primitives — spheres, capsules, boxes, capped cylinders and bones (a capsule between the
 * origins of two body rows) — each attached to a row of a pose tensor in the Isaac Gym [N, B, 13] layout (position 0:3, quaternion
 * xyzw 3:7), or world-fixed (row -1).  What is drawn is the project's own UNVERIFIED collision geometry plus a stick figure of the
 * body tree: no meshes, no textures; anti-aliasing is opt-in supersampling (pp_render_rays_aa).
 *
 * Two launches per picture:
 *   pp_render_pose   render_pose_kernel: one workgroup per selected env, lane p places primitive p in world space and writes
 *                    posed[E][P] to global memory (callers and tests can read it).
 *   pp_render_rays   render_rays_kernel<1>: grid = image tiles x selected envs, a 16 x 16 pixel tile per 256-lane workgroup (a wave
 *                    owns a 16 x 4 strip).  The workgroup copies its env's posed primitives into LDS; every lane intersects its
 *                    ray with all of them and the ground plane, keeps the nearest hit, shades
 *                        albedo * (ambient + diffuse * max(n . l, 0) * shadow)
 *                    with one any-hit shadow ray towards the light (from the hit point, offset PP_RENDER_SHADOW_OFFSET along the
 *                    normal) and stores one RGBA8 pixel as a single 4-byte store: channel = (int)(255 * clamp(v, 0, 1) + 0.5),
 *                    alpha 255.  Lanes of a ragged tile that fall outside the image store nothing.
 *   pp_render_rays_aa  instead of pp_render_rays: pixel (x, y) is the box mean of s x s rays through (x + (i + 1/2) / s, y + (j + 1/2) / s),
 *                    i, j = 0 .. s - 1, s = `samples` = 1, 2 or 4.  Each ray is shaded as above and its three channels are clamped to [0, 1];
 *                    the s^2 colours are added in ONE fixed order (a binary tree over k = j * s + i: ppenv_render_device.h,
 *                    render_aa_tree_sum), the sum is multiplied by the exact 1 / s^2 and channel = (int)(255 v + 0.5), alpha 255.
 *                    render_rays_kernel<s>: the same workgroup over a 16 x 16 tile of SUB-SAMPLES — s^2 consecutive lanes own a pixel, one
 *                    ray each, added across lanes in that order; the pixel's first lane stores the 4 bytes.  samples = 1 launches
 *                    render_rays_kernel<1>: the bytes of pp_render_rays.  RGBA only: a mean of depths or ids has no meaning.
 * A recording (deferred capture): the posed list is a complete, camera-independent description of a frame, 80 bytes per primitive.
 *   pp_render_pose_anchor  instead of pp_render_pose (render_pose_kernel with an anchor array): the same bytes into posed_out[count][P], plus anchor_out[count] as float4 — words 0 .. 2 of
 *                    body row `anchor_row` of pose source `anchor_source` of that env, then 0 (zeros for anchor_row < 0 and for an env id out of
 *                    range).  The caller keeps a ring of such slots.
 *   pp_render_rays_frames  posed [F][E][P] + anchor [F][E] -> rgba [F, E, H, W, 4] in ONE launch of the same render_rays_kernel<s>, grid (image
 *                    tiles, E, F): per workgroup what pp_render_rays (samples 1) / pp_render_rays_aa (2, 4) do for one env of one picture (their
 *                    grid is this one with F = 1), so frame f is byte for byte the picture those entries draw from posed[f].  The one difference: a following camera
 *                    (follow_row >= 0; follow_source is ignored) adds (anchor.x, anchor.y, 0) of that frame and env.  The scene's source[] is never
 *                    read and may be empty (num_sources 0): a replay has no task.  RGBA only.
 * Images are [E, H, W, 4] uint8; the optional outputs are [E, H, W] fp32 depth (distance along the ray, +inf for sky) and int32
 * primitive id (PP_RENDER_ID_SKY, PP_RENDER_ID_GROUND, or the primitive's index).
 *
 * The env selection is a DEVICE array of at most PP_RENDER_MAX_ENVS env ids; an id outside [0, num_envs) draws an empty scene
 * (sky and ground) instead of reading out of bounds.  No atomics, no cross-workgroup communication: every pixel and every posed
 * primitive is a pure function of the inputs, so two renders of one state are bitwise equal.
 *
 * Plain C, device pointers, caller's HIP stream, no synchronisation (pp_render_scene_upload alone copies host memory: once per
 * scene); returns 0 or a negative PPENV_E* code (ppenv.h) with the message in ppenv_last_error().
 */
#ifndef PPENV_RENDER_H
#define PPENV_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_RENDER_MAX_PRIMS 160
#define PP_RENDER_MAX_ENVS 16
#define PP_RENDER_MAX_SOURCES 4
#define PP_RENDER_TILE_W 16
#define PP_RENDER_TILE_H 16
#define PP_RENDER_SHADOW_OFFSET 1e-3f                 /* metres along the normal */
#define PP_RENDER_T_MIN 1e-4f                         /* hits nearer than this along a ray are ignored */

#define PP_RENDER_SPHERE 0                            /* a: centre */
#define PP_RENDER_CAPSULE 1                           /* a, b: end points of the axis */
#define PP_RENDER_BOX 2                               /* a: centre, b: half extents along the body frame's axes */
#define PP_RENDER_CYLINDER 3                          /* a, b: centres of the two flat caps */
#define PP_RENDER_BONE 4                              /* a capsule from the origin of `row` to the origin of `row2` (a, b unused) */

#define PP_RENDER_ID_SKY (-1)
#define PP_RENDER_ID_GROUND (-2)

/* One pose tensor: element k of row r of env e is base[e * env_stride + r * row_stride + k] (strides in floats). */
typedef struct pp_render_source {
    const float* base;
    int64_t env_stride;
    int64_t row_stride;
    int32_t rows;                                     /* rows per env: what `row` / `row2` are checked against */
    int32_t reserved;
} pp_render_source;

typedef struct pp_render_prim {
    int32_t kind;                                     /* PP_RENDER_SPHERE .. PP_RENDER_BONE */
    int32_t source;                                   /* index into pp_render_scene.source (ignored when row < 0) */
    int32_t row;                                      /* -1: a, b are world coordinates */
    int32_t row2;                                     /* bones only */
    float a[3];
    float b[3];
    float radius;
    float albedo[3];
} pp_render_prim;

/* A primitive placed in world space: 20 words. */
typedef struct pp_render_posed {
    float a[3];
    float radius;
    float b[3];
    int32_t kind;                                     /* a bone has become PP_RENDER_CAPSULE; -1: nothing (env id out of range) */
    float axis[9];                                    /* boxes: the three unit axes, one after the other */
    float albedo[3];
} pp_render_posed;

typedef struct pp_render_scene {
    int32_t num_envs;                                 /* envs in every source tensor */
    int32_t num_prims;
    int32_t num_sources;
    int32_t checker;                                  /* 0: the ground has colour ground_rgb[0] everywhere */
    pp_render_source source[PP_RENDER_MAX_SOURCES];
    float ground_z;
    float checker_pitch;
    float ground_rgb[2][3];
    float sky_rgb[3];
    float light[3];                                   /* unit vector TOWARDS the light */
    float ambient;
    float diffuse;
} pp_render_scene;

typedef struct pp_render_camera {
    float eye[3];
    float target[3];
    float up[3];
    float fov_deg;                                    /* vertical field of view */
    int32_t width;
    int32_t height;
    int32_t follow_source;                            /* with follow_row >= 0: that body's x and y (not z) are added to eye and target, */
    int32_t follow_row;                               /* per env, on the device; -1: a fixed camera */
} pp_render_camera;

/* Checks `scene` and its `prims` (host memory, scene->num_prims of them) and copies the primitives to prims_dev. */
int pp_render_scene_upload(const pp_render_scene* scene, const pp_render_prim* prims, pp_render_prim* prims_dev, void* stream);

/* Launch 1.  env_ids: device, count of them (1 .. PP_RENDER_MAX_ENVS); posed: device, [count][scene->num_prims]. */
int pp_render_pose(const pp_render_scene* scene, const pp_render_prim* prims_dev, const int32_t* env_ids, int32_t count, pp_render_posed* posed,
                   void* stream);

/* Launch 2.  rgba [count, H, W, 4] uint8, 4-byte aligned; depth [count, H, W] f32 and ids [count, H, W] i32 may be NULL. */
int pp_render_rays(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids, int32_t count,
                   uint8_t* rgba, float* depth, int32_t* ids, void* stream);

/* Launch 2, supersampled: `samples` sub-samples per axis, 1, 2 or 4 (anything else: PPENV_EINVAL); rgba as for pp_render_rays. */
int pp_render_rays_aa(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids, int32_t count,
                      int32_t samples, uint8_t* rgba, void* stream);

/* Launch 1 of a recording: pp_render_pose + anchor_out [count][4] f32 (16-byte aligned).  anchor_row < 0: zeros; otherwise checked like a
 * camera's follow row. */
int pp_render_pose_anchor(const pp_render_scene* scene, const pp_render_prim* prims_dev, const int32_t* env_ids, int32_t count, int32_t anchor_source,
                          int32_t anchor_row, pp_render_posed* posed_out, float* anchor_out, void* stream);

/* All rays of `frames` recorded frames.  posed [frames][count][scene->num_prims]; anchor [frames][count][4] f32, 16-byte aligned (may be NULL
 * under a fixed camera); rgba [frames, count, H, W, 4] uint8, 4-byte aligned.  samples 1, 2 or 4; frames 1 .. 65535 and fewer than 2^32 lanes
 * (256 per 16 x 16 tile of rays) in the launch — a longer recording is cast in several calls over consecutive frame ranges. */
int pp_render_rays_frames(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const float* anchor, int32_t frames,
                          int32_t count, int32_t samples, uint8_t* rgba, void* stream);

#ifdef __cplusplus
}
#endif

#endif
