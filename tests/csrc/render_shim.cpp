// render_shim.cpp — the ray caster's per-primitive and per-pixel arithmetic (isaacgym_amd/csrc/ppenv_render_device.h) compiled for the
// host, as play_shim.cpp does for the episode accounting.  TEST INFRASTRUCTURE ONLY.  Built by tests/render_shim_binding.py with
// -ffp-contract=off and WITHOUT -ffinite-math-only (the depth of a sky pixel is +inf).
#include "../../isaacgym_amd/csrc/ppenv_render_device.h"

extern "C" {

size_t render_shim_sizeof_prim() { return sizeof(pp_render_prim); }
size_t render_shim_sizeof_posed() { return sizeof(pp_render_posed); }
size_t render_shim_sizeof_scene() { return sizeof(pp_render_scene); }
size_t render_shim_sizeof_camera() { return sizeof(pp_render_camera); }

// render_pose_kernel on host memory: posed[count][num_prims]
void render_shim_pose(const pp_render_scene* sc, const pp_render_prim* prims, const int32_t* env_ids, int32_t count, pp_render_posed* posed) {
    for (int32_t s = 0; s < count; ++s)
        for (int32_t p = 0; p < sc->num_prims; ++p) {
            pp_render_posed& out = posed[(size_t)s * sc->num_prims + p];
            if (env_ids[s] >= 0 && env_ids[s] < sc->num_envs) pp::render_place(*sc, prims[p], env_ids[s], out);
            else pp::render_place_none(out);
        }
}

// render_rays_kernel<1> on host memory, pixel by pixel; shadow / parity [count, H, W] i32 are the shim's own extra outputs (may be NULL)
void render_shim_rays(const pp_render_scene* sc, const pp_render_camera* cam, const pp_render_posed* posed, const int32_t* env_ids, int32_t count,
                      uint32_t* rgba, float* depth, int32_t* ids, int32_t* shadow, int32_t* parity) {
    pp::RenderView view;
    pp::render_view_of(*cam, view);
    for (int32_t s = 0; s < count; ++s) {
        const bool ok = env_ids[s] >= 0 && env_ids[s] < sc->num_envs;
        const pp::V3 follow = ok ? pp::render_follow(*sc, view, env_ids[s]) : pp::mk(0.0f, 0.0f, 0.0f);
        for (int32_t y = 0; y < cam->height; ++y)
            for (int32_t x = 0; x < cam->width; ++x) {
                const pp::RenderPixel px = pp::render_pixel(*sc, view, follow, posed + (size_t)s * sc->num_prims, sc->num_prims, (float)x + 0.5f, (float)y + 0.5f);
                const size_t at = ((size_t)s * cam->height + y) * cam->width + x;
                rgba[at] = px.rgba;
                if (depth) depth[at] = px.depth;
                if (ids) ids[at] = px.id;
                if (shadow) shadow[at] = px.shadow;
                if (parity) parity[at] = px.parity;
            }
    }
}

}
