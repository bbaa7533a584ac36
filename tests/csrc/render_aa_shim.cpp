// render_aa_shim.cpp — the supersampled pixel of the ray caster (isaacgym_amd/csrc/ppenv_render_device.h: render_pixel_aa) compiled for the
// host, next to render_shim.cpp's one-ray pixel.  TEST INFRASTRUCTURE ONLY.  Built by tests/render_aa_shim_binding.py with the flags of
// render_shim_binding: -ffp-contract=off and WITHOUT -ffinite-math-only.
#include "../../isaacgym_amd/csrc/ppenv_render_device.h"

extern "C" {

// render_rays_kernel<S> on host memory, pixel by pixel: rgba [count, H, W] words.  -> 0, or -1 for samples other than 1, 2, 4
int render_aa_shim_rays(const pp_render_scene* sc, const pp_render_camera* cam, const pp_render_posed* posed, const int32_t* env_ids, int32_t count,
                        int32_t samples, uint32_t* rgba) {
    if (!pp::render_samples_ok(samples)) return -1;
    pp::RenderView view;
    pp::render_view_of(*cam, view);
    for (int32_t s = 0; s < count; ++s) {
        const bool ok = env_ids[s] >= 0 && env_ids[s] < sc->num_envs;
        const pp::V3 follow = ok ? pp::render_follow(*sc, view, env_ids[s]) : pp::mk(0.0f, 0.0f, 0.0f);
        for (int32_t y = 0; y < cam->height; ++y)
            for (int32_t x = 0; x < cam->width; ++x)
                rgba[((size_t)s * cam->height + y) * cam->width + x] =
                    pp::render_pixel_aa(*sc, view, follow, posed + (size_t)s * sc->num_prims, sc->num_prims, x, y, samples);
    }
    return 0;
}

// render_aa_tree_sum on n = 1, 4 or 16 values of one channel: the order of the sum, for the test that restates it
float render_aa_shim_tree_sum(const float* v, int32_t n) {
    pp::V3 c[pp::kRenderMaxSamples * pp::kRenderMaxSamples];
    for (int32_t k = 0; k < n; ++k) c[k] = pp::mk(v[k], 0.0f, 0.0f);
    return pp::render_aa_tree_sum(c, n).x;
}

}
