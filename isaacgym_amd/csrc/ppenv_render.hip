// ppenv_render.hip — the ray caster's two kernels and entry points (include/ppenv_render.h; arithmetic: ppenv_render_device.h).
//
//   render_pose_kernel      one workgroup per selected env, lane p places primitive p: posed[E][P] in global memory.  With an anchor array lane 0
//                           also writes one float4 per env: words 0 .. 2 of the anchor row (what a following camera adds to eye and target), so a
//                           recorded frame needs no pose tensor later.
//   render_rays_kernel<S>   grid (image tiles, selected envs, frames) over posed[F][E][P], 256 lanes = a 16 x 16 tile of rays (a wave owns a 16 x 4
//                           strip).  The workgroup copies its slot's posed primitives into LDS word by word (at most 160 x 20 words = 12.5 KiB), then
//                           every lane walks the same list for its own ray — the LDS reads are wave-uniform broadcasts.
//                           S = 1: a ray is a pixel; the lane stores its 4 bytes and, when asked, depth and id.
//                           S = 2, 4: the tile is one of SUB-SAMPLES: S x S consecutive lanes own one pixel, one ray each; their clamped colours are
//                           added by a butterfly of log2(S^2) __shfl_xor steps per channel in the order render_aa_tree_sum fixes, and the pixel's
//                           first lane stores the 4 bytes.  A wave still owns a 16 x 4 strip of rays, so a supersampled picture has S^2 times the
//                           waves of the plain one (300 workgroups at 320 x 240 become 1200 / 4800) instead of S^2 sequential rays per lane.
//                           `follow` comes from the live pose tensor through env_ids (the eager entries: one frame) or, without env_ids, from
//                           anchor[F][E] (a whole recording in one launch; sc.source is never touched).
// A picture is bound by the intersection arithmetic (pixels x primitives x 2 rays), not by bytes: 640 x 480 x 4 B out, a few KiB in.
// No atomics, no cross-workgroup communication; the only divergence is the per-lane choice of primitive kind and the shadow ray.
//
// -ffinite-math-only is NOT in this unit's flags (isaacgym_amd/_lib.py): the depth of a sky pixel is +inf.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ppenv_render_device.h"

#include "ppenv_host.h"

namespace {

constexpr int kTileW = PP_RENDER_TILE_W, kTileH = PP_RENDER_TILE_H;
constexpr int kBlock = kTileW * kTileH;
constexpr int kPosedWords = sizeof(pp_render_posed) / 4;
static_assert(sizeof(pp_render_posed) == 80 && kBlock == 256 && PP_RENDER_MAX_PRIMS <= kBlock, "layout of include/ppenv_render.h");

// anchor (may be NULL): lane 0 also writes (row[0], row[1], row[2], 0) of body `anchor_row`, zeros without one or for an env id out of range.
__global__ __launch_bounds__(kBlock) void render_pose_kernel(const pp_render_scene sc, const pp_render_prim* __restrict__ prims,
                                                             const int32_t* __restrict__ env_ids, int32_t anchor_source, int32_t anchor_row,
                                                             pp_render_posed* __restrict__ posed, float4* __restrict__ anchor) {
    const int32_t p = (int32_t)threadIdx.x;
    const int32_t env = env_ids[blockIdx.x];
    const bool ok = env >= 0 && env < sc.num_envs;
    if (p == 0 && anchor) {
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok && anchor_row >= 0) {
            const float* r = pp::render_row(sc.source[anchor_source], env, anchor_row);
            a = make_float4(r[0], r[1], r[2], 0.0f);
        }
        anchor[blockIdx.x] = a;
    }
    if (p >= sc.num_prims) return;
    pp_render_posed out;
    if (ok) pp::render_place(sc, prims[p], env, out);
    else pp::render_place_none(out);
    posed[(size_t)blockIdx.x * sc.num_prims + p] = out;
}

// Frame blockIdx.z, env blockIdx.y.  Lane tid -> pixel tid / S^2 of a (16 / S) x (16 / S) pixel tile, sub-sample tid % S^2 (render_aa_sample's k): the
// S^2 lanes of a pixel are consecutive and never straddle a wave, and they leave together on a ragged tile, so the butterfly only ever reads lanes
// that are active.  `follow` is settled before the barrier, the same way by the whole workgroup: env_ids given, the live body row of that env (zero
// for an id out of range); else anchor[slot] under a following camera (anchor may be NULL under a fixed one).
template <int S>
__global__ __launch_bounds__(kBlock) void render_rays_kernel(const pp_render_scene sc, const pp::RenderView view, const pp_render_posed* __restrict__ posed,
                                                             const int32_t* __restrict__ env_ids, const float4* __restrict__ anchor, int32_t tiles_x,
                                                             uint32_t* __restrict__ rgba, float* __restrict__ depth, int32_t* __restrict__ ids) {
    constexpr int kSub = S * S, kPixW = kTileW / S, kPixH = kTileH / S;
    static_assert((S == 1 || S == 2 || S == 4) && kTileW % S == 0 && kTileH % S == 0, "sub-samples per axis: a power of two inside a wave");
    __shared__ pp_render_posed lds[PP_RENDER_MAX_PRIMS];
    const int tid = (int)threadIdx.x;
    const size_t slot = (size_t)blockIdx.z * gridDim.y + blockIdx.y;          // [frame][env]
    pp::V3 follow = pp::mk(0.0f, 0.0f, 0.0f);
    if (env_ids) {
        const int32_t env = env_ids[slot];
        if (env >= 0 && env < sc.num_envs) follow = pp::render_follow(sc, view, env);
    } else if (view.follow_row >= 0) {
        const float4 a = anchor[slot];
        follow = pp::mk(a.x, a.y, 0.0f);
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(posed + slot * sc.num_prims);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
        for (int w = tid; w < sc.num_prims * kPosedWords; w += kBlock) dst[w] = src[w];
    }
    __syncthreads();
    const int pix = tid / kSub, k = tid % kSub;
    const int32_t x = (int32_t)(blockIdx.x % tiles_x) * kPixW + pix % kPixW;
    const int32_t y = (int32_t)(blockIdx.x / tiles_x) * kPixH + pix / kPixW;
    if (x >= view.width || y >= view.height) return;         // ragged tiles: after the barrier, all lanes of a pixel together
    const size_t at = (slot * view.height + y) * view.width + x;
    if constexpr (S == 1) {
        const pp::RenderPixel px = pp::render_pixel(sc, view, follow, lds, sc.num_prims, (float)x + 0.5f, (float)y + 0.5f);
        rgba[at] = px.rgba;
        if (depth) depth[at] = px.depth;
        if (ids) ids[at] = px.id;
    } else {
        pp::V3 c = pp::render_aa_sample(sc, view, follow, lds, sc.num_prims, x, y, S, k);
#pragma unroll
        for (int m = 1; m < kSub; m *= 2) {                  // render_aa_tree_sum's levels
            c.x += __shfl_xor(c.x, m);
            c.y += __shfl_xor(c.y, m);
            c.z += __shfl_xor(c.z, m);
        }
        if (k == 0) rgba[at] = pp::render_aa_pack(c, S);
    }
}

bool count_ok(int32_t count, const char* who) {
    if (count >= 1 && count <= PP_RENDER_MAX_ENVS) return true;
    pp_set_errorf("%s: the env selection must have 1 .. %d entries", who, PP_RENDER_MAX_ENVS);
    return false;
}

// the header alone (the primitives were checked when they were uploaded)
bool scene_ok(const pp_render_scene* sc, const char* who) {
    if (sc->num_prims < 0 || sc->num_prims > PP_RENDER_MAX_PRIMS) {
        pp_set_errorf("%s: more than PP_RENDER_MAX_PRIMS (%d) primitives, or a negative count", who, PP_RENDER_MAX_PRIMS);
        return false;
    }
    if (sc->num_envs <= 0 || sc->num_sources < 0 || sc->num_sources > PP_RENDER_MAX_SOURCES) {
        pp_set_errorf("%s: num_envs must be positive and num_sources 0 .. %d", who, PP_RENDER_MAX_SOURCES);
        return false;
    }
    for (int32_t s = 0; s < sc->num_sources; ++s)
        if (!sc->source[s].base || sc->source[s].rows <= 0) {
            pp_set_errorf("%s: pose source %d has a NULL base or no rows", who, s);
            return false;
        }
    return true;
}

bool row_ok(const pp_render_scene* sc, int32_t source, int32_t row) {
    return source >= 0 && source < sc->num_sources && row >= 0 && row < sc->source[source].rows;
}

}  // namespace

extern "C" int pp_render_scene_upload(const pp_render_scene* scene, const pp_render_prim* prims, pp_render_prim* prims_dev, void* stream) {
    if (!scene || !prims || !prims_dev) {
        ppenv_set_error("pp_render_scene_upload: NULL pointer");
        return PPENV_EINVAL;
    }
    if (!scene_ok(scene, "pp_render_scene_upload")) return PPENV_EINVAL;
    for (int32_t i = 0; i < scene->num_prims; ++i) {
        const pp_render_prim& p = prims[i];
        if (p.kind < PP_RENDER_SPHERE || p.kind > PP_RENDER_BONE || !(p.radius >= 0.0f)) {
            pp_set_errorf("pp_render_scene_upload: primitive %d has an unknown kind or a negative radius", i);
            return PPENV_EINVAL;
        }
        const bool bone = p.kind == PP_RENDER_BONE;
        if ((bone || p.row >= 0) && (!row_ok(scene, p.source, p.row) || (bone && !row_ok(scene, p.source, p.row2))) || p.row < -1) {
            pp_set_errorf("pp_render_scene_upload: primitive %d: source or row out of range", i);
            return PPENV_EINVAL;
        }
    }
    if (scene->num_prims > 0)
        PP_HIP(hipMemcpyAsync(prims_dev, prims, (size_t)scene->num_prims * sizeof(pp_render_prim), hipMemcpyHostToDevice, (hipStream_t)stream));
    return PPENV_OK;
}

namespace {

// the one pose launch; anchor_out NULL: no anchors
int launch_pose(const pp_render_scene* scene, const pp_render_prim* prims_dev, const int32_t* env_ids, int32_t count, int32_t anchor_source,
                int32_t anchor_row, pp_render_posed* posed, float* anchor_out, void* stream) {
    hipLaunchKernelGGL(render_pose_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, *scene, prims_dev, env_ids, anchor_source, anchor_row, posed,
                       reinterpret_cast<float4*>(anchor_out));
    return pp_launched("launching render_pose_kernel failed");
}

bool camera_ok(const pp_render_camera* camera, const char* who) {
    if (camera->width > 0 && camera->height > 0 && camera->width <= 16384 && camera->height <= 16384 && camera->fov_deg > 0.0f && camera->fov_deg < 180.0f) return true;
    pp_set_errorf("%s: width and height must be positive (at most 16384) and the field of view inside (0, 180) degrees", who);
    return false;
}

// what pp_render_rays and pp_render_rays_aa check alike
bool rays_ok(const char* who, const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids,
             int32_t count, const uint8_t* rgba) {
    if (!scene || !camera || !posed || !env_ids || !rgba) {
        pp_set_errorf("%s: NULL pointer", who);
        return false;
    }
    if (!count_ok(count, who) || !scene_ok(scene, who) || !camera_ok(camera, who)) return false;
    if (camera->follow_row >= 0 && !row_ok(scene, camera->follow_source, camera->follow_row)) {
        pp_set_errorf("%s: the camera's follow source or row is out of range", who);
        return false;
    }
    if ((uintptr_t)rgba % 4 != 0) {
        pp_set_errorf("%s: rgba must be 4-byte aligned", who);
        return false;
    }
    return true;
}

// The one ray launch, arguments checked by the entry: posed [frames][count][P] -> rgba [frames, count, H, W, 4], `follow` from env_ids (frames 1) or
// from anchor.  limits_who: refuse, in that entry's name, what one grid cannot hold (z at most 65535, x below 2^31, fewer than 2^32 lanes in all).
int launch_rays(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids, const float* anchor,
                int32_t frames, int32_t count, int32_t samples, uint8_t* rgba, float* depth, int32_t* ids, void* stream, const char* limits_who) {
    const int32_t pw = kTileW / samples, ph = kTileH / samples;                                                       // pixels per workgroup
    const int64_t tiles_x = (camera->width + pw - 1) / pw, tiles_y = (camera->height + ph - 1) / ph;
    if (limits_who && (frames > 65535 || tiles_x * tiles_y * (int64_t)count * frames * kBlock >= ((int64_t)1 << 32))) {
        pp_set_errorf("%s: %d frames of %d x %d pictures of %d envs with %d x %d samples exceed one launch's grid (65535 frames, 2^32 lanes): split the frames",
                      limits_who, frames, camera->width, camera->height, count, samples, samples);
        return PPENV_EINVAL;
    }
    pp::RenderView view;
    pp::render_view_of(*camera, view);
    const auto kernel = samples == 1 ? render_rays_kernel<1> : samples == 2 ? render_rays_kernel<2> : render_rays_kernel<4>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)(tiles_x * tiles_y), (uint32_t)count, (uint32_t)frames), dim3(kBlock), 0, (hipStream_t)stream, *scene, view, posed,
                       env_ids, reinterpret_cast<const float4*>(anchor), (int32_t)tiles_x, reinterpret_cast<uint32_t*>(rgba), depth, ids);
    return pp_launched("launching render_rays_kernel failed");
}

}  // namespace

extern "C" int pp_render_pose(const pp_render_scene* scene, const pp_render_prim* prims_dev, const int32_t* env_ids, int32_t count,
                              pp_render_posed* posed, void* stream) {
    if (!scene || !prims_dev || !env_ids || !posed) {
        ppenv_set_error("pp_render_pose: NULL pointer");
        return PPENV_EINVAL;
    }
    if (!count_ok(count, "pp_render_pose") || !scene_ok(scene, "pp_render_pose")) return PPENV_EINVAL;
    if (scene->num_prims == 0) return PPENV_OK;
    return launch_pose(scene, prims_dev, env_ids, count, 0, -1, posed, nullptr, stream);
}

extern "C" int pp_render_rays(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids,
                              int32_t count, uint8_t* rgba, float* depth, int32_t* ids, void* stream) {
    if (!rays_ok("pp_render_rays", scene, camera, posed, env_ids, count, rgba)) return PPENV_EINVAL;
    return launch_rays(scene, camera, posed, env_ids, nullptr, 1, count, 1, rgba, depth, ids, stream, nullptr);
}

extern "C" int pp_render_rays_aa(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids,
                                 int32_t count, int32_t samples, uint8_t* rgba, void* stream) {
    if (!rays_ok("pp_render_rays_aa", scene, camera, posed, env_ids, count, rgba)) return PPENV_EINVAL;
    if (!pp::render_samples_ok(samples)) {
        pp_set_errorf("pp_render_rays_aa: samples per axis must be 1, 2 or 4, got %d", samples);
        return PPENV_EINVAL;
    }
    return launch_rays(scene, camera, posed, env_ids, nullptr, 1, count, samples, rgba, nullptr, nullptr, stream, nullptr);     // one sample: pp_render_rays' bytes
}

extern "C" int pp_render_pose_anchor(const pp_render_scene* scene, const pp_render_prim* prims_dev, const int32_t* env_ids, int32_t count,
                                     int32_t anchor_source, int32_t anchor_row, pp_render_posed* posed_out, float* anchor_out, void* stream) {
    if (!scene || !prims_dev || !env_ids || !posed_out || !anchor_out) {
        ppenv_set_error("pp_render_pose_anchor: NULL pointer");
        return PPENV_EINVAL;
    }
    if (!count_ok(count, "pp_render_pose_anchor") || !scene_ok(scene, "pp_render_pose_anchor")) return PPENV_EINVAL;
    if (anchor_row >= 0 && !row_ok(scene, anchor_source, anchor_row)) {
        ppenv_set_error("pp_render_pose_anchor: the anchor's source or row is out of range");
        return PPENV_EINVAL;
    }
    if ((uintptr_t)anchor_out % 16 != 0) {
        ppenv_set_error("pp_render_pose_anchor: anchor_out must be 16-byte aligned");
        return PPENV_EINVAL;
    }
    return launch_pose(scene, prims_dev, env_ids, count, anchor_source, anchor_row, posed_out, anchor_out, stream);
}

extern "C" int pp_render_rays_frames(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const float* anchor,
                                     int32_t frames, int32_t count, int32_t samples, uint8_t* rgba, void* stream) {
    const char* who = "pp_render_rays_frames";
    if (!scene || !camera || !posed || !rgba) {
        pp_set_errorf("%s: NULL pointer", who);
        return PPENV_EINVAL;
    }
    if (!count_ok(count, who)) return PPENV_EINVAL;
    if (frames < 1) {
        pp_set_errorf("%s: frames must be positive, got %d", who, frames);
        return PPENV_EINVAL;
    }
    if (!pp::render_samples_ok(samples)) {
        pp_set_errorf("%s: samples per axis must be 1, 2 or 4, got %d", who, samples);
        return PPENV_EINVAL;
    }
    // the header's constants alone: a replay has no pose tensor (num_sources 0, NULL bases), and none is read here
    if (scene->num_prims < 0 || scene->num_prims > PP_RENDER_MAX_PRIMS || scene->num_sources < 0 || scene->num_sources > PP_RENDER_MAX_SOURCES) {
        pp_set_errorf("%s: num_prims must be 0 .. %d and num_sources 0 .. %d", who, PP_RENDER_MAX_PRIMS, PP_RENDER_MAX_SOURCES);
        return PPENV_EINVAL;
    }
    if (!camera_ok(camera, who)) return PPENV_EINVAL;
    if (camera->follow_row >= 0 && !anchor) {
        pp_set_errorf("%s: a following camera needs the anchor array", who);
        return PPENV_EINVAL;
    }
    if ((uintptr_t)rgba % 4 != 0 || (uintptr_t)anchor % 16 != 0) {
        pp_set_errorf("%s: rgba must be 4-byte aligned and anchor 16-byte aligned", who);
        return PPENV_EINVAL;
    }
    return launch_rays(scene, camera, posed, nullptr, anchor, frames, count, samples, rgba, nullptr, nullptr, stream, who);
}
