"""What every ABI entry answers to a NULL handle or descriptor: the return code and the exact ppenv_last_error() text.

These answers come from argument validation alone, before the entry touches the HIP runtime, so the library gives them on a machine
without a GPU.  Every other argument is zero / NULL as well.  The table was typed in from what the library returned when this test
was written; host-side changes of the library must leave it as it is.

Left out: no entry of include/*.h that takes a handle or a descriptor starts with a HIP call.  The entries without one have nothing
to refuse here: ppenv_abi_version, ppenv_last_error, and the size queries that take only counts (ppenv_dr_state_bytes,
ppenv_dr_state_draws_offset, ppenv_mlp_chain_workspace_bytes, ppenv_mlp_bias_grad_workspace_bytes,
ppenv_running_mean_std_workspace_bytes, ppenv_ppo_loss_partial_floats, ppenv_play_partial_bytes)."""
import ctypes as C

import pytest

from isaacgym_amd import _lib

EINVAL, EHIP = -1, -3
NULL_ARG = "NULL argument"

# entry -> (return code, ppenv_last_error() text)
REFUSED = {
    # ---- include/ppenv.h
    "ppenv_create": (EINVAL, "out is NULL"),
    "ppenv_buffers_of": (EINVAL, NULL_ARG),
    "ppenv_config_of": (EINVAL, NULL_ARG),
    "ppenv_step": (EINVAL, NULL_ARG),
    "ppenv_step_into": (EINVAL, NULL_ARG),
    "ppenv_step_sequence": (EINVAL, "NULL argument or negative count"),
    "ppenv_reset_all": (EINVAL, NULL_ARG),
    "ppenv_reduce_stats": (EINVAL, NULL_ARG),
    "ppenv_reset_idx": (EINVAL, "ppenv_reset_idx: NULL ids or negative count"),
    "ppenv_pd_targets": (EINVAL, NULL_ARG),
    "ppenv_serve_from_draws": (EINVAL, "NULL argument or m <= 0"),
    "ppenv_set_randomization": (EINVAL, NULL_ARG),
    "ppenv_set_gravity": (EINVAL, NULL_ARG),
    "ppenv_post_physics_step": (EINVAL, NULL_ARG),
    "ppenv_refresh_root_states": (EINVAL, NULL_ARG),
    "ppenv_refresh_dof_states": (EINVAL, NULL_ARG),
    "ppenv_refresh_dof_force": (EINVAL, NULL_ARG),
    "ppenv_refresh_rigid_body_states": (EINVAL, NULL_ARG),
    "ppenv_set_serve_override": (EINVAL, NULL_ARG),
    "ppenv_get_state": (EINVAL, NULL_ARG),
    "ppenv_set_state": (EINVAL, NULL_ARG),
    "ppenv_ta_post_physics_step": (EINVAL, "ppenv_ta_post_physics_step: NULL argument or num_envs <= 0"),
    "ppenv_t4_rewards": (EINVAL, "ppenv_t4_rewards: NULL argument or num_envs <= 0"),
    "ppenv_ta_sim_create": (EINVAL, "ppenv_ta_sim_create: NULL argument"),
    "ppenv_ta_sim_set_gravity": (EINVAL, "ppenv_ta_sim_set_gravity: NULL handle"),
    "ppenv_ta_sim_set_policy_input": (EINVAL, "ppenv_ta_sim_set_policy_input: NULL handle"),
    "ppenv_ta_sim_set_randomization": (EINVAL, "ppenv_ta_sim_set_randomization: NULL handle"),
    "ppenv_ta_model_is_compiled": (EINVAL, ""),
    "ppenv_ta_simulate": (EINVAL, "ppenv_ta_simulate: NULL argument or num_envs <= 0"),
    "ppenv_ta_forward_kinematics": (EINVAL, "ppenv_ta_forward_kinematics: NULL argument or num_envs <= 0"),
    "ppenv_ta_step": (EINVAL, "ppenv_ta_step: NULL argument or num_envs <= 0"),
    "ppenv_ta_pd_targets": (EINVAL, "ppenv_ta_pd_targets: NULL argument or num_envs <= 0"),
    "ppenv_ta_serve_from_draws": (EINVAL, "ppenv_ta_serve_from_draws: NULL argument or m <= 0"),
    # ---- include/ppenv_dr.h
    "ppenv_dr_plan_upload": (EINVAL, "ppenv_dr_plan_upload: NULL pointer, num_envs <= 0, frequency < 1, reset_rows not 1 or 2, not 1..8 tables, or an entry with a "
                                     "NULL table, rows outside 1..64, an unknown distribution / operation / schedule or a schedule without its schedule_steps"),
    "ppenv_dr_apply": (EINVAL, "ppenv_dr_apply: NULL pointer or num_envs <= 0"),
    "ppenv_dr_apply_ids": (EINVAL, "ppenv_dr_apply_ids: NULL pointer, num_envs <= 0 or count < 0"),
    # ---- include/ppenv_policy.h
    "ppenv_mlp_layer_forward": (EINVAL, "ppenv_mlp_layer_forward: NULL pointer or inconsistent sizes (need lda >= k, ldw >= k, ldo >= n)"),
    "ppenv_mlp_layer_forward_share": (EINVAL, "ppenv_mlp_layer_forward: NULL pointer or inconsistent sizes (need lda >= k, ldw >= k, ldo >= n)"),
    "ppenv_mlp_chain_forward": (EINVAL, "ppenv_mlp_chain_forward: 2 .. 4 layers and a 4-byte aligned workspace of ppenv_mlp_chain_workspace_bytes (zeroed once, by the caller)"),
    "ppenv_mlp_chain_status": (EHIP, "ppenv_mlp_chain_status: NULL or unreadable workspace"),
    "ppenv_mlp_prepare_input": (EINVAL, "ppenv_mlp_prepare_input: NULL pointer or inconsistent sizes (need ld_obs >= k, ld_out >= k and a multiple of 8, out 16-byte aligned, "
                                        "mean and inv_std together)"),
    "ppenv_mlp_sample_actions": (EINVAL, "ppenv_mlp_sample_actions: NULL pointer or inconsistent sizes (need 0 < a <= 256, ld_mu >= a)"),
    "ppenv_mlp_heads_sample": (EINVAL, "ppenv_mlp_heads_sample: needs a heads layer the skinny kernel takes (fp16 input, fp32 output, batch 1, n <= 32, k % 16 == 0, "
                                       "16-byte aligned rows) and 0 < num_actions <= n"),
    "ppenv_gae": (EINVAL, "ppenv_gae: NULL pointer or non-positive size"),
    "ppenv_mlp_layer_backward_input": (EINVAL, "ppenv_mlp_layer_backward_input: the descriptor must have bias NULL, elu 0 and an fp16 output"),
    "ppenv_mlp_layer_backward_weight": (EINVAL, "ppenv_mlp_layer_backward_weight: NULL pointer or inconsistent sizes (need lddz >= n, ldx >= k, lddw >= k)"),
    "ppenv_mlp_reduce_rows": (EINVAL, "ppenv_mlp_reduce_rows: NULL pointer or inconsistent sizes"),
    "ppenv_mlp_bias_grad_f32": (EINVAL, "ppenv_mlp_bias_grad_f32: NULL pointer or inconsistent sizes"),
    "ppenv_mlp_cast_weights": (EINVAL, "ppenv_mlp_cast_weights: NULL pointer or inconsistent sizes (need ldw32 >= k, ldw16 >= k, ldwt16 >= n, wt_rows >= k)"),
    "ppenv_mlp_cast_weights_batch": (EINVAL, "ppenv_mlp_cast_weights_batch: NULL items or count outside 1 .. 32"),
    "ppenv_running_mean_std_update": (EINVAL, "ppenv_running_mean_std_update: NULL pointer or inconsistent sizes (need ld >= k, k <= 16256, an 8-byte aligned workspace of "
                                              "ppenv_running_mean_std_workspace_bytes() whose first 1024 bytes were zeroed once)"),
    # ---- include/ppenv_ppo.h
    "ppenv_ppo_loss_grad": (EINVAL, "ppenv_ppo_loss_grad: NULL pointer or inconsistent sizes (need 0 < a <= 32, row strides >= a, ld_d_head >= a + 1)"),
    "ppenv_ppo_grad_sumsq": (EINVAL, "ppenv_ppo_grad_sumsq: NULL pointer, 0 < count <= 64 tensors, 0 < parts <= 65535"),
    "ppenv_ppo_adam_step": (EINVAL, "ppenv_ppo_adam_step: NULL pointer, state_in == state_out (the state is double-buffered), bad sizes or world < 0"),
    # ---- include/ppenv_play.h
    "ppenv_play_reset": (EINVAL, "ppenv_play_reset: NULL pointer, num_envs <= 0, num_agents not 1 or 2, or more than 2^31 - 1 rows"),
    "ppenv_play_accumulate": (EINVAL, "ppenv_play_accumulate: NULL pointer, num_envs <= 0, num_agents not 1 or 2, more than 2^31 - 1 rows, or games_num < 1"),
}

# entries that answer NULL with a value instead of an error, and leave ppenv_last_error() alone
ANSWERED = {
    "ppenv_status": 0, "ppenv_step_kernel_name": b"", "ppenv_state_bytes": 0, "ppenv_arena_bytes": 0, "ppenv_mlp_dw_workspace_bytes": 0,
    "ppenv_ta_sim_device": -1, "ppenv_ta_sim_status": 0, "ppenv_ta_sim_kernel": -1, "ppenv_ta_sim_kernel_name": b"",
    "ppenv_destroy": None, "ppenv_ta_sim_destroy": None,
}


def _zeros(fn):
    """NULL for every pointer, zero for every number, a zeroed struct for one passed by value."""
    return [None if issubclass(t, (C.c_void_p, C._Pointer)) else t() if issubclass(t, C.Structure) else 0 for t in fn.argtypes]


def _poison(L, name):
    """Leave a known, different text in ppenv_last_error() so that the next call's own text (an empty one included) shows."""
    if name == "ppenv_gae":
        assert L.ppenv_ta_sim_set_gravity(None, 0.0, None) == EINVAL
    else:
        assert L.ppenv_gae(*_zeros(L.ppenv_gae)) == EINVAL
    return L.ppenv_last_error()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_null_is_refused_with_the_pinned_code_and_text(name):
    L = _lib.lib()
    rc, text = REFUSED[name]
    assert _poison(L, name).decode() != text
    fn = getattr(L, name)
    assert fn(*_zeros(fn)) == rc
    assert L.ppenv_last_error().decode() == text


@pytest.mark.parametrize("name", sorted(ANSWERED))
def test_null_is_answered_without_an_error(name):
    L = _lib.lib()
    before = _poison(L, name)
    fn = getattr(L, name)
    assert fn(*_zeros(fn)) == ANSWERED[name]
    assert L.ppenv_last_error() == before


def test_create_refuses_a_null_config_before_the_runtime():
    L = _lib.lib()
    out = C.c_void_p(0x1)
    _poison(L, "ppenv_create")
    assert L.ppenv_create(None, None, 0, None, C.byref(out)) == EINVAL
    assert L.ppenv_last_error().decode() == "config is NULL"
    assert out.value is None


def test_ta_sim_create_unwinds_a_handle_it_refuses_before_the_runtime(monkeypatch):
    """Two refusals that come after the handle was allocated and before any HIP call: a model the constants cannot be made from,
    and PPENV_TA_KERNEL=chain with a model other than the compiled one."""
    from isaacgym_amd import scene
    L = _lib.lib()
    sc = scene.build_ta_scene(1)
    bad, other = scene.build_ta_model(), scene.build_ta_model()
    bad.num_contacts = -1
    other.link[3].mass *= 2
    for model, kernel, text in ((bad, None, "ppenv_ta_sim_create: num_contacts out of range"),
                                (other, "chain", "PPENV_TA_KERNEL=chain, but the model differs from the one compiled into the chain-wave kernel "
                                                 "(run python -m isaacgym_amd.modelgen_ta and rebuild)")):
        if kernel:
            monkeypatch.setenv("PPENV_TA_KERNEL", kernel)
        out = C.c_void_p(0x1)
        assert L.ppenv_ta_sim_create(C.byref(sc), C.byref(model), None, C.byref(out)) == EINVAL
        assert L.ppenv_last_error().decode() == text
        assert out.value is None


def test_every_bound_entry_is_in_one_table_or_named_as_left_out():
    L = _lib.lib()
    left_out = {"ppenv_abi_version", "ppenv_last_error", "ppenv_dr_state_bytes", "ppenv_dr_state_draws_offset", "ppenv_mlp_chain_workspace_bytes",
                "ppenv_mlp_bias_grad_workspace_bytes", "ppenv_running_mean_std_workspace_bytes", "ppenv_ppo_loss_partial_floats", "ppenv_play_partial_bytes"}
    bound = {n for n in vars(L) if n.startswith("ppenv_")}
    assert len(bound) >= 76
    assert bound == set(REFUSED) | set(ANSWERED) | left_out
