// ppenv_render.hip — the ray caster's two kernels and entry points (include/ppenv_render.h; arithmetic: ppenv_render_device.h).
//
//   render_pose_kernel   one workgroup per selected env, lane p places primitive p: posed[E][P] in global memory.
//   render_rays_kernel   grid (image tiles, selected envs), 256 lanes = a 16 x 16 pixel tile (a wave owns a 16 x 4 strip).  The workgroup
//                        copies its env's posed primitives into LDS word by word (at most 160 x 20 words = 12.5 KiB), then every lane
//                        walks the same list for its own ray — the LDS reads are wave-uniform broadcasts — and stores one 4-byte pixel.
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

__global__ __launch_bounds__(kBlock) void render_pose_kernel(const pp_render_scene sc, const pp_render_prim* __restrict__ prims,
                                                             const int32_t* __restrict__ env_ids, pp_render_posed* __restrict__ posed) {
    const int32_t p = (int32_t)threadIdx.x;
    if (p >= sc.num_prims) return;
    const int32_t env = env_ids[blockIdx.x];
    pp_render_posed out;
    if (env >= 0 && env < sc.num_envs) pp::render_place(sc, prims[p], env, out);
    else pp::render_place_none(out);
    posed[(size_t)blockIdx.x * sc.num_prims + p] = out;
}

__global__ __launch_bounds__(kBlock) void render_rays_kernel(const pp_render_scene sc, const pp::RenderView view, const pp_render_posed* __restrict__ posed,
                                                             const int32_t* __restrict__ env_ids, int32_t tiles_x, uint32_t* __restrict__ rgba,
                                                             float* __restrict__ depth, int32_t* __restrict__ ids) {
    __shared__ pp_render_posed lds[PP_RENDER_MAX_PRIMS];
    const int tid = (int)threadIdx.x;
    const int32_t sel = (int32_t)blockIdx.y;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(posed + (size_t)sel * sc.num_prims);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
        for (int w = tid; w < sc.num_prims * kPosedWords; w += kBlock) dst[w] = src[w];
    }
    __syncthreads();
    const int32_t x = (int32_t)(blockIdx.x % tiles_x) * kTileW + (tid & (kTileW - 1));
    const int32_t y = (int32_t)(blockIdx.x / tiles_x) * kTileH + tid / kTileW;
    if (x >= view.width || y >= view.height) return;         // ragged tiles: after the barrier
    const int32_t env = env_ids[sel];
    const bool ok = env >= 0 && env < sc.num_envs;
    const pp::V3 follow = ok ? pp::render_follow(sc, view, env) : pp::mk(0.0f, 0.0f, 0.0f);
    const pp::RenderPixel px = pp::render_pixel(sc, view, follow, lds, sc.num_prims, (float)x + 0.5f, (float)y + 0.5f);
    const size_t at = ((size_t)sel * view.height + y) * view.width + x;
    rgba[at] = px.rgba;
    if (depth) depth[at] = px.depth;
    if (ids) ids[at] = px.id;
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

extern "C" int pp_render_pose(const pp_render_scene* scene, const pp_render_prim* prims_dev, const int32_t* env_ids, int32_t count,
                              pp_render_posed* posed, void* stream) {
    if (!scene || !prims_dev || !env_ids || !posed) {
        ppenv_set_error("pp_render_pose: NULL pointer");
        return PPENV_EINVAL;
    }
    if (!count_ok(count, "pp_render_pose") || !scene_ok(scene, "pp_render_pose")) return PPENV_EINVAL;
    if (scene->num_prims == 0) return PPENV_OK;
    hipLaunchKernelGGL(render_pose_kernel, dim3(count), dim3(kBlock), 0, (hipStream_t)stream, *scene, prims_dev, env_ids, posed);
    return pp_launched("launching render_pose_kernel failed");
}

extern "C" int pp_render_rays(const pp_render_scene* scene, const pp_render_camera* camera, const pp_render_posed* posed, const int32_t* env_ids,
                              int32_t count, uint8_t* rgba, float* depth, int32_t* ids, void* stream) {
    if (!scene || !camera || !posed || !env_ids || !rgba) {
        ppenv_set_error("pp_render_rays: NULL pointer");
        return PPENV_EINVAL;
    }
    if (!count_ok(count, "pp_render_rays") || !scene_ok(scene, "pp_render_rays")) return PPENV_EINVAL;
    if (camera->width <= 0 || camera->height <= 0 || camera->width > 16384 || camera->height > 16384 || !(camera->fov_deg > 0.0f) || !(camera->fov_deg < 180.0f)) {
        ppenv_set_error("pp_render_rays: width and height must be positive (at most 16384) and the field of view inside (0, 180) degrees");
        return PPENV_EINVAL;
    }
    if (camera->follow_row >= 0 && !row_ok(scene, camera->follow_source, camera->follow_row)) {
        ppenv_set_error("pp_render_rays: the camera's follow source or row is out of range");
        return PPENV_EINVAL;
    }
    if ((uintptr_t)rgba % 4 != 0) {
        ppenv_set_error("pp_render_rays: rgba must be 4-byte aligned");
        return PPENV_EINVAL;
    }
    pp::RenderView view;
    pp::render_view_of(*camera, view);
    const int32_t tiles_x = (camera->width + kTileW - 1) / kTileW, tiles_y = (camera->height + kTileH - 1) / kTileH;
    hipLaunchKernelGGL(render_rays_kernel, dim3(tiles_x * tiles_y, count), dim3(kBlock), 0, (hipStream_t)stream, *scene, view, posed, env_ids, tiles_x,
                       reinterpret_cast<uint32_t*>(rgba), depth, ids);
    return pp_launched("launching render_rays_kernel failed");
}
