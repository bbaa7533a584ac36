"""Loader of the HIP library `isaacgym_amd/lib/libppenv.so` and the one ctypes binding of its C ABI (include/*.h): `load()`.

There is no CPU fallback: if the library is missing or does not load, importing the
environment fails loudly.  `build()` compiles it with hipcc for gfx950 (cross-compiles
without a GPU); the built .so lives in-tree so it travels with the source snapshot.
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import torch

from . import scene

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("PPENV_LIB", os.path.join(_PKG, "lib", "libppenv.so"))   # PPENV_LIB: profiling builds only
SOURCES = [os.path.join(_PKG, "csrc", "ppenv.hip"), os.path.join(_PKG, "csrc", "ppenv_ta.hip"), os.path.join(_PKG, "csrc", "ppenv_ta_sim.hip"),
           os.path.join(_PKG, "csrc", "ppenv_ta_chain.hip"), os.path.join(_PKG, "csrc", "ppenv_policy.hip"), os.path.join(_PKG, "csrc", "ppenv_policy_bwd.hip"),
           os.path.join(_PKG, "csrc", "ppenv_ppo.hip"), os.path.join(_PKG, "csrc", "ppenv_dr.hip"), os.path.join(_PKG, "csrc", "ppenv_play.hip"),
           os.path.join(_PKG, "csrc", "ppenv_ppo_meter.hip"), os.path.join(_PKG, "csrc", "ppenv_render.hip"), os.path.join(_PKG, "csrc", "ppenv_serve.hip"),
           os.path.join(_PKG, "csrc", "ppenv_play_pair.hip"), os.path.join(_PKG, "csrc", "ppenv_play_act.hip"),
           os.path.join(_PKG, "csrc", "ppenv_play_delay.hip"), os.path.join(_PKG, "csrc", "ppenv_train_delay.hip"),
           os.path.join(_PKG, "csrc", "ppenv_serve_curric.hip"), os.path.join(_PKG, "csrc", "ppenv_dr_adr.hip"),
           os.path.join(_PKG, "csrc", "ppenv_critic_input.hip"), os.path.join(_PKG, "csrc", "ppenv_history.hip"),
           os.path.join(_PKG, "csrc", "ppenv_sensor.hip")]
HEADERS = [os.path.join(_PKG, "csrc", "ppenv_device.h"), os.path.join(_PKG, "csrc", "ppenv_model_g1.h"), os.path.join(_PKG, "csrc", "ppenv_ta_device.h"), os.path.join(_PKG, "csrc", "ppenv_ta_task.h"), os.path.join(_PKG, "csrc", "ppenv_ta_chain.h"), os.path.join(_PKG, "csrc", "ppenv_model_g1_ta.h"),
           os.path.join(ROOT, "include", "ppenv.h"), os.path.join(ROOT, "include", "ppenv_policy.h"), os.path.join(ROOT, "include", "ppenv_ppo.h"),
           os.path.join(_PKG, "csrc", "ppenv_dr_device.h"), os.path.join(ROOT, "include", "ppenv_dr.h"),
           os.path.join(_PKG, "csrc", "ppenv_play_device.h"), os.path.join(ROOT, "include", "ppenv_play.h"), os.path.join(ROOT, "include", "ppenv_play_group.h"),
           os.path.join(_PKG, "csrc", "ppenv_ppo_meter_device.h"), os.path.join(ROOT, "include", "ppenv_ppo_meter.h"),
           os.path.join(_PKG, "csrc", "ppenv_render_device.h"), os.path.join(ROOT, "include", "ppenv_render.h"),
           os.path.join(_PKG, "csrc", "ppenv_ta_outcome_device.h"), os.path.join(ROOT, "include", "ppenv_ta_outcome.h"),
           os.path.join(_PKG, "csrc", "ppenv_serve_device.h"), os.path.join(ROOT, "include", "ppenv_serve.h"),
           os.path.join(_PKG, "csrc", "ppenv_play_pair_device.h"), os.path.join(ROOT, "include", "ppenv_play_pair.h"),
           os.path.join(_PKG, "csrc", "ppenv_play_act_device.h"), os.path.join(ROOT, "include", "ppenv_play_act.h"),
           os.path.join(_PKG, "csrc", "ppenv_play_delay_device.h"), os.path.join(ROOT, "include", "ppenv_play_delay.h"),
           os.path.join(_PKG, "csrc", "ppenv_train_delay_device.h"), os.path.join(ROOT, "include", "ppenv_train_delay.h"),
           os.path.join(_PKG, "csrc", "ppenv_serve_curric_device.h"), os.path.join(ROOT, "include", "ppenv_serve_curric.h"),
           os.path.join(_PKG, "csrc", "ppenv_dr_adr_device.h"), os.path.join(ROOT, "include", "ppenv_dr_adr.h"),
           os.path.join(_PKG, "csrc", "ppenv_critic_input_device.h"), os.path.join(ROOT, "include", "ppenv_critic_input.h"),
           os.path.join(_PKG, "csrc", "ppenv_history_device.h"), os.path.join(ROOT, "include", "ppenv_history.h"),
           os.path.join(_PKG, "csrc", "ppenv_sensor_device.h"), os.path.join(ROOT, "include", "ppenv_sensor.h"),
           os.path.join(_PKG, "csrc", "ppenv_host.h"), os.path.join(_PKG, "csrc", "ppenv_reduce_device.h"), os.path.join(_PKG, "csrc", "ppenv_play_host.h")]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-mllvm", "-disable-vector-combine", "-fno-signed-zeros", "-ffinite-math-only", "-fPIC", "-shared"]
# per translation unit, after HIPCC_FLAGS: the optimizer's step skip must see an inf / nan gradient norm; the play totals' minima / maxima start at +-inf;
# the score meter's fp64 update rounds every operation on its own, as its host build does (no contraction, signed zeros, a nan mean stays one);
# the ray caster's depth of a sky pixel is +inf; the serve plan's draw rounds every operation on its own, as its host build does, and a pinned zero keeps its sign;
# the paired statistics round d * d before adding it, as their host build does, and their table starts as NaN;
# the actuator accounting rounds t * t and t * v before adding them, as its host build does, and its largest excursion starts at -inf;
# the serve curriculum draws with the serve plan's arithmetic and rounds every fp64 operation of its table on its own, as its host build does;
# ADR draws with the reset-time plan's arithmetic, stages returns as the serve curriculum does and rounds every operation of its update on its own;
# the privileged critic inputs copy a float bit for bit (a negative zero keeps its sign) and round the normaliser's two operations on their own;
# the observation and action history moves words bit for bit, and its clamp keeps a negative zero's sign and turns a NaN action into lo;
# the sensor line rounds s * g before adding it, and its level draws' product before their sum, as its host build does, and a row of zero amplitude copies bits
SOURCE_FLAGS = {"ppenv_ppo.hip": ["-fno-finite-math-only"], "ppenv_play.hip": ["-fno-finite-math-only"], "ppenv_render.hip": ["-fno-finite-math-only"],
                "ppenv_ppo_meter.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_serve.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_serve_curric.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_dr_adr.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_critic_input.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_history.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_sensor.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_play_pair.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"],
                "ppenv_play_act.hip": ["-fno-finite-math-only", "-fsigned-zeros", "-ffp-contract=off"]}

_lib = None


class PPEnvError(RuntimeError):
    pass


# ---- ctypes mirrors of the structs load() binds (policy, ppo and play re-export theirs; include/ppenv.h's and ppenv_dr.h's live in scene)
class MLPLayer(C.Structure):
    """ctypes mirror of ppenv_mlp_layer (include/ppenv_policy.h)."""
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("batch", C.c_int32),
                ("in_", C.c_void_p), ("in_stride", C.c_int64), ("lda", C.c_int32), ("in_f32", C.c_int32),
                ("mean", C.c_void_p), ("inv_std", C.c_void_p), ("clip", C.c_float),
                ("w", C.c_void_p), ("w_stride", C.c_int64), ("ldw", C.c_int32),
                ("bias", C.c_void_p), ("bias_stride", C.c_int64), ("elu", C.c_int32),
                ("out", C.c_void_p), ("out_stride", C.c_int64), ("ldo", C.c_int32), ("out_f32", C.c_int32)]


class MLPDw(C.Structure):
    """ctypes mirror of ppenv_mlp_dw (include/ppenv_policy.h)."""
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("batch", C.c_int32),
                ("dz", C.c_void_p), ("dz_stride", C.c_int64), ("lddz", C.c_int32),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("ldx", C.c_int32),
                ("dw", C.c_void_p), ("dw_stride", C.c_int64), ("lddw", C.c_int32),
                ("accumulate", C.c_int32), ("splits", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class MLPCast(C.Structure):
    """ctypes mirror of ppenv_mlp_cast (include/ppenv_policy.h)."""
    _fields_ = [("w32", C.c_void_p), ("n", C.c_int32), ("k", C.c_int32), ("ldw32", C.c_int32),
                ("w16", C.c_void_p), ("ldw16", C.c_int32),
                ("wt16", C.c_void_p), ("ldwt16", C.c_int32), ("wt_rows", C.c_int32)]


class PPOLossArgs(C.Structure):
    """ctypes mirror of ppenv_ppo_loss_args (include/ppenv_ppo.h)."""
    _fields_ = [("m", C.c_int32), ("a", C.c_int32),
                ("mu", C.c_void_p), ("ld_mu", C.c_int32), ("value", C.c_void_p), ("ld_value", C.c_int32),
                ("actions", C.c_void_p), ("ld_actions", C.c_int32), ("old_mu", C.c_void_p), ("ld_old_mu", C.c_int32),
                ("old_sigma", C.c_void_p), ("old_neglogp", C.c_void_p), ("advantages", C.c_void_p), ("old_values", C.c_void_p),
                ("returns", C.c_void_p), ("logstd", C.c_void_p),
                ("e_clip", C.c_float), ("critic_coef", C.c_float), ("bounds_loss_coef", C.c_float), ("soft_bound", C.c_float),
                ("entropy_coef", C.c_float), ("clip_value", C.c_int32), ("scale", C.c_void_p),
                ("d_head", C.c_void_p), ("ld_d_head", C.c_int32), ("d_logstd", C.c_void_p), ("stats", C.c_void_p), ("partial", C.c_void_p)]


class PPOTensor(C.Structure):
    """ctypes mirror of ppenv_ppo_tensor."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p),
                ("rows", C.c_int32), ("cols", C.c_int32), ("ld_p", C.c_int32), ("ld_g", C.c_int32)]


class PPOAdam(C.Structure):
    """ctypes mirror of ppenv_ppo_adam."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("max_norm", C.c_float), ("truncate", C.c_int32),
                ("growth_factor", C.c_float), ("backoff_factor", C.c_float), ("growth_interval", C.c_int32), ("world", C.c_int32)]


MAX_AGENTS = 2                             # PPENV_PLAY_MAX_AGENTS


class PlayTotals(C.Structure):
    """ctypes mirror of ppenv_play_totals (include/ppenv_play.h)."""
    _fields_ = [("games", C.c_int64), ("steps", C.c_int64), ("launches", C.c_int64),
                ("reward", C.c_double * MAX_AGENTS), ("reward_sq", C.c_double * MAX_AGENTS),
                ("reward_min", C.c_float * MAX_AGENTS), ("reward_max", C.c_float * MAX_AGENTS)]


class PlayPairTotals(C.Structure):
    """ctypes mirror of pp_play_pair_totals (include/ppenv_play_pair.h)."""
    _fields_ = [("pairs", C.c_int64), ("steps_diff", C.c_int64), ("diff", C.c_double * MAX_AGENTS), ("diff_sq", C.c_double * MAX_AGENTS),
                ("cell", C.c_double * MAX_AGENTS), ("base", C.c_double * MAX_AGENTS)]


PLAY_ACT_MAX_DOF, PLAY_ACT_FIELDS = 32, 10                                               # PP_PLAY_ACT_MAX_DOF, PP_PLAY_ACT_FIELDS
PLAY_DELAY_MAX, PLAY_DELAY_MAX_WIDTH = 15, 512                                           # PP_PLAY_DELAY_MAX, PP_PLAY_DELAY_MAX_WIDTH


class TrainDelayConsts(C.Structure):
    """ctypes mirror of pp_train_delay_consts (include/ppenv_train_delay.h)."""
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32), ("seed", C.c_uint64), ("env_id_offset", C.c_int32), ("channel", C.c_int32)]


class SensorConsts(C.Structure):
    """ctypes mirror of pp_sensor_consts (include/ppenv_sensor.h)."""
    _fields_ = [("sigma_lo", C.c_float), ("sigma_hi", C.c_float), ("drop_lo", C.c_float), ("drop_hi", C.c_float), ("draw", C.c_int32), ("seed", C.c_uint64),
                ("env_id_offset", C.c_int32), ("key_period", C.c_int32), ("channel", C.c_int32)]


class PlayActLimit(C.Structure):
    """ctypes mirror of pp_play_act_limit (include/ppenv_play_act.h)."""
    _fields_ = [("lower", C.c_float), ("upper", C.c_float), ("effort", C.c_float), ("vel_limit", C.c_float)]


class PlayActThresholds(C.Structure):
    """ctypes mirror of pp_play_act_thresholds."""
    _fields_ = [("effort_frac", C.c_float), ("vel_frac", C.c_float), ("limit_margin", C.c_float), ("action_clip", C.c_float)]


class PlayActInput(C.Structure):
    """ctypes mirror of pp_play_act_input: value (e, d) = p[e * env_stride + d * dof_stride], strides in elements."""
    _fields_ = [("p", C.c_void_p), ("env_stride", C.c_int64), ("dof_stride", C.c_int64)]


class PlayActInputs(C.Structure):
    """ctypes mirror of pp_play_act_inputs."""
    _fields_ = [("q", PlayActInput), ("qd", PlayActInput), ("tau", PlayActInput), ("action", PlayActInput)]


class PlayActGroup(C.Structure):
    """ctypes mirror of pp_play_act_group."""
    _fields_ = [("games", C.c_int64), ("samples", C.c_int64), ("launches", C.c_int64), ("energy", C.c_double), ("energy_sq", C.c_double)]


class PlayActJoint(C.Structure):
    """ctypes mirror of pp_play_act_joint."""
    _fields_ = [("c_effort", C.c_int64), ("c_vel", C.c_int64), ("c_limit", C.c_int64), ("c_clip", C.c_int64),
                ("abs_tau", C.c_double), ("tau_sq", C.c_double), ("power", C.c_double),
                ("max_abs_tau", C.c_float), ("max_abs_vel", C.c_float), ("max_exc", C.c_float), ("reserved", C.c_float)]


class PPOMeter(C.Structure):
    """ctypes mirror of ppenv_ppo_meter (include/ppenv_ppo_meter.h)."""
    _fields_ = [("mean_reward", C.c_double), ("mean_length", C.c_double), ("current_size", C.c_int64), ("games_total", C.c_int64),
                ("updates", C.c_int64)]


TA_OUTCOME_NAMES = ("closer", "hit_paddle", "cross_net", "hit_table", "fall_down")      # PP_TA_OUTCOME_*: the bits 16 .. 256 of the TA flags


class TAOutcome(C.Structure):
    """ctypes mirror of pp_ta_outcome (include/ppenv_ta_outcome.h): 16 words of 8 bytes."""
    _fields_ = [("windows", C.c_uint64), ("envs", C.c_uint64), ("count", C.c_uint64 * 5), ("last_envs", C.c_uint64), ("last", C.c_uint64 * 5),
                ("reserved", C.c_uint64 * 3)]


SERVE_LAYOUT_SOA3, SERVE_LAYOUT_AOS5 = 0, 1                                              # PP_SERVE_LAYOUT_*
SERVE_MAX_TILT_DEG = 57.0                                                               # PP_SERVE_MAX_TILT_DEG


class ServeCell(C.Structure):
    """ctypes mirror of pp_serve_cell (include/ppenv_serve.h)."""
    _fields_ = [("speed_lo", C.c_float), ("speed_hi", C.c_float), ("tilt_lo_deg", C.c_float), ("tilt_hi_deg", C.c_float),
                ("tilt_z_lo_deg", C.c_float), ("tilt_z_hi_deg", C.c_float), ("ball_y_lo", C.c_float), ("ball_y_hi", C.c_float),
                ("ball_z_lo", C.c_float), ("ball_z_hi", C.c_float)]


class ServePlan(C.Structure):
    """ctypes mirror of pp_serve_plan."""
    _fields_ = [("num_envs", C.c_int32), ("env_id_offset", C.c_int32), ("seed", C.c_uint64), ("form", C.c_int32), ("layout", C.c_int32),
                ("reset_rows", C.c_int32), ("groups", C.c_int32), ("envs_per_group", C.c_int32), ("paired", C.c_int32), ("cells", C.c_void_p)]


CURRIC_MAX_BINS, CURRIC_MAX_POWER, CURRIC_FOLD_CHUNK = 256, 4, 16384                     # PP_CURRIC_MAX_BINS, PP_CURRIC_MAX_POWER, PP_CURRIC_FOLD_CHUNK
CURRIC_DROPPED = -2 ** 63                                                               # PP_CURRIC_DROPPED


class ServeCurric(C.Structure):
    """ctypes mirror of pp_serve_curric (include/ppenv_serve_curric.h)."""
    _fields_ = [("num_envs", C.c_int32), ("env_id_offset", C.c_int32), ("seed", C.c_uint64), ("form", C.c_int32), ("layout", C.c_int32),
                ("reset_rows", C.c_int32), ("num_agents", C.c_int32), ("bins", C.c_int32), ("power", C.c_int32), ("mix", C.c_float),
                ("alpha", C.c_float), ("cells", C.c_void_p)]


class ServeCurricState(C.Structure):
    """ctypes mirror of pp_serve_curric_state: device pointers."""
    _fields_ = [("count", C.c_void_p), ("next_bin", C.c_void_p), ("cur_bin", C.c_void_p), ("ret", C.c_void_p), ("games", C.c_void_p),
                ("mean", C.c_void_p), ("dropped", C.c_void_p), ("cdf", C.c_void_p)]


ADR_COIN_INDEX, ADR_PICK_INDEX, ADR_MAX_SLOTS = 512, 513, 2 * scene.DR_MAX_TABLES + 1     # PP_ADR_COIN_INDEX, PP_ADR_PICK_INDEX, PP_ADR_MAX_SLOTS


class AdrDim(C.Structure):
    """ctypes mirror of pp_dr_adr_dim (include/ppenv_dr_adr.h)."""
    _fields_ = [("table", C.c_void_p), ("rows", C.c_int32), ("start_lo", C.c_float), ("start_hi", C.c_float), ("limit_lo", C.c_float),
                ("limit_hi", C.c_float), ("step", C.c_float)]


class Adr(C.Structure):
    """ctypes mirror of pp_dr_adr."""
    _fields_ = [("num_envs", C.c_int32), ("env_id_offset", C.c_int32), ("seed", C.c_uint64), ("reset_rows", C.c_int32), ("num_agents", C.c_int32),
                ("dims", C.c_int32), ("thr", C.c_uint32), ("min_games", C.c_int32), ("t_low", C.c_float), ("t_high", C.c_float), ("reserved", C.c_int32),
                ("dim", AdrDim * scene.DR_MAX_TABLES)]


class AdrState(C.Structure):
    """ctypes mirror of pp_dr_adr_state: device pointers."""
    _fields_ = [("range", C.c_void_p), ("draws", C.c_void_p), ("slot", C.c_void_p), ("ret", C.c_void_p), ("acc_n", C.c_void_p), ("acc_q", C.c_void_p),
                ("games", C.c_void_p), ("dropped", C.c_void_p), ("mean", C.c_void_p), ("widened", C.c_void_p), ("narrowed", C.c_void_p)]


CRITIC_MAX_SOURCES, CRITIC_MAX_COLS = 16, 1024                                           # PP_CRITIC_MAX_SOURCES, PP_CRITIC_MAX_COLS
CRITIC_F32, CRITIC_I32, CRITIC_ROW_MAJOR, CRITIC_TABLE_MAJOR = 0, 1, 0, 1                # PP_CRITIC_F32 / _I32, PP_CRITIC_ROW_MAJOR / _TABLE_MAJOR
HISTORY_MAX, HISTORY_MAX_WIDTH = 8, 16256                                                # PP_HISTORY_MAX, PP_HISTORY_MAX_WIDTH


class CriticSource(C.Structure):
    """ctypes mirror of pp_critic_source (include/ppenv_critic_input.h)."""
    _fields_ = [("p", C.c_void_p), ("kind", C.c_int32), ("cols", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32), ("stride", C.c_int64)]


class CriticTable(C.Structure):
    """ctypes mirror of pp_critic_table."""
    _fields_ = [("rows", C.c_int32), ("num_agents", C.c_int32), ("sources", C.c_int32), ("total_cols", C.c_int32), ("source", CriticSource * CRITIC_MAX_SOURCES)]


RENDER_MAX_PRIMS, RENDER_MAX_ENVS, RENDER_MAX_SOURCES = 160, 16, 4           # PP_RENDER_MAX_*
RENDER_SPHERE, RENDER_CAPSULE, RENDER_BOX, RENDER_CYLINDER, RENDER_BONE = range(5)
RENDER_ID_SKY, RENDER_ID_GROUND = -1, -2


class RenderSource(C.Structure):
    """ctypes mirror of pp_render_source (include/ppenv_render.h)."""
    _fields_ = [("base", C.c_void_p), ("env_stride", C.c_int64), ("row_stride", C.c_int64), ("rows", C.c_int32), ("reserved", C.c_int32)]


class RenderPrim(C.Structure):
    """ctypes mirror of pp_render_prim."""
    _fields_ = [("kind", C.c_int32), ("source", C.c_int32), ("row", C.c_int32), ("row2", C.c_int32), ("a", C.c_float * 3), ("b", C.c_float * 3),
                ("radius", C.c_float), ("albedo", C.c_float * 3)]


class RenderPosed(C.Structure):
    """ctypes mirror of pp_render_posed: 20 words."""
    _fields_ = [("a", C.c_float * 3), ("radius", C.c_float), ("b", C.c_float * 3), ("kind", C.c_int32), ("axis", C.c_float * 9), ("albedo", C.c_float * 3)]


class RenderScene(C.Structure):
    """ctypes mirror of pp_render_scene."""
    _fields_ = [("num_envs", C.c_int32), ("num_prims", C.c_int32), ("num_sources", C.c_int32), ("checker", C.c_int32),
                ("source", RenderSource * RENDER_MAX_SOURCES), ("ground_z", C.c_float), ("checker_pitch", C.c_float),
                ("ground_rgb", (C.c_float * 3) * 2), ("sky_rgb", C.c_float * 3), ("light", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float)]


class RenderCamera(C.Structure):
    """ctypes mirror of pp_render_camera."""
    _fields_ = [("eye", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3), ("fov_deg", C.c_float), ("width", C.c_int32),
                ("height", C.c_int32), ("follow_source", C.c_int32), ("follow_row", C.c_int32)]


def is_stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in SOURCES + HEADERS)


def build(force=False, verbose=False, out=None, extra_flags=(), extra_deps=()):
    """hipcc --offload-arch=gfx950 -> isaacgym_amd/lib/libppenv.so.  out / extra_flags: a build of the same sources for another
    compiled-in arm model (-DPPENV_MODEL_HEADER=..., see build_for_arm_model) — loaded with load(), never the default library."""
    out = LIB_PATH if out is None else out
    if not force and os.path.exists(out):
        t = os.path.getmtime(out)
        if not any(os.path.getmtime(p) > t for p in SOURCES + HEADERS + list(extra_deps)):
            return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    tmp = f"{out}.{os.getpid()}.tmp"          # built aside and renamed: another process never sees half a library
    objdir = tempfile.mkdtemp(prefix="ppenv_build_")
    compile_flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags)

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        cmd = [hipcc] + compile_flags + SOURCE_FLAGS.get(os.path.basename(src), []) + ["-c", "-o", obj, src]
        return obj, cmd, subprocess.run(cmd, capture_output=True, text=True)
    try:
        with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as pool:      # one translation unit per core
            done = list(pool.map(compile_one, SOURCES))
        for obj, cmd, res in done:
            if res.returncode != 0:
                raise PPEnvError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stderr[-4000:])
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + [obj for obj, _, _ in done]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise PPEnvError("hipcc (link) failed:\n" + " ".join(cmd) + "\n" + res.stderr[-4000:])
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
        shutil.rmtree(objdir, ignore_errors=True)
    if verbose:
        print(" ".join(cmd))
    return out


def build_for_arm_model(config, out_dir, force=False):
    """The library with ANOTHER 7-dof arm compiled in: `config` carries the model (scene.build_config after
    scene.use_arm_tables(urdf.arm_specs(...))); modelgen writes its header into out_dir and the same sources are built against it.
    -> path of out_dir/libppenv.so (load it with load(); ppenv_create of THAT library accepts the config, the default one refuses it)."""
    from . import modelgen
    os.makedirs(out_dir, exist_ok=True)
    header = os.path.join(out_dir, "ppenv_model.h")
    text = modelgen.generate(config)
    if not os.path.exists(header) or open(header).read() != text:
        with open(header, "w") as fh:
            fh.write(text)
    return build(force=force, out=os.path.join(out_dir, "libppenv.so"), extra_flags=[f'-DPPENV_MODEL_HEADER="{header}"'], extra_deps=[header])


def build_for_ta_model(model, out_dir, scene_cfg=None, force=False):
    """The library with ANOTHER 27-dof tree compiled into the chain-wave kernel (TA:470 `g1_27dof.urdf`): `model` is a
    scene.TAModel (isaacgym_amd.urdf.ta_model of the asset), `scene_cfg` the scene whose collision shapes ride on it (default
    scene.build_ta_scene).  modelgen_ta writes the tree's header into out_dir and the same sources are built against it
    (-DPPENV_TA_MODEL_HEADER=...): ppenv_ta_sim_create of THAT library then selects ta_chain_kernel for the model — the default
    library keeps its table-driven kernels for it (and refuses PPENV_TA_KERNEL=chain).  The tree must have the G1's topology: limbs of
    6 + 6 + 3 + 7 + 5 links on the pelvis / torso; anything else fails the kernel's static_asserts at compile time, not at run time.
    -> path of out_dir/libppenv.so (load()).  The 7-dof kernels of that library carry the stock arm."""
    from . import modelgen_ta
    os.makedirs(out_dir, exist_ok=True)
    header = os.path.join(out_dir, "ppenv_model_ta.h")
    text = modelgen_ta.generate(scene_cfg if scene_cfg is not None else scene.build_ta_scene(1), model)
    if not os.path.exists(header) or open(header).read() != text:
        with open(header, "w") as fh:
            fh.write(text)
    return build(force=force, out=os.path.join(out_dir, "libppenv.so"), extra_flags=[f'-DPPENV_TA_MODEL_HEADER="{header}"'], extra_deps=[header])


def lib():
    """The loaded library with argtypes set.  Raises PPEnvError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PPEnvError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (needs hipcc). There is no CPU fallback.")
    _lib = load(LIB_PATH)
    return _lib


def load(path):
    """A libppenv build with EVERY function of include/*.h bound (lib() for the default one; build_for_arm_model's or build_for_ta_model's
    output for another model).  This is the only place that sets argtypes / restype: an unbound function would take a device pointer
    as a C int and truncate it without an error."""
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise PPEnvError(f"could not load {path}: {e}") from e
    L.ppenv_abi_version.argtypes = []
    if L.ppenv_abi_version() != scene.ABI_VERSION:
        raise PPEnvError("libppenv.so ABI version does not match isaacgym_amd.scene; rebuild the library")
    vp, sz, i32, i64, u64, f32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_uint64, C.c_float
    cfgp, layerp = C.POINTER(scene.Config), C.POINTER(MLPLayer)
    # ---- include/ppenv.h
    L.ppenv_last_error.restype = C.c_char_p
    L.ppenv_last_error.argtypes = []
    L.ppenv_arena_bytes.restype = sz
    L.ppenv_arena_bytes.argtypes = [cfgp]
    L.ppenv_create.argtypes = [cfgp, vp, sz, vp, C.POINTER(vp)]
    L.ppenv_destroy.restype = None
    L.ppenv_destroy.argtypes = [vp]
    L.ppenv_buffers_of.argtypes = [vp, C.POINTER(scene.Buffers)]
    L.ppenv_config_of.argtypes = [vp, cfgp]
    L.ppenv_step.argtypes = [vp, vp, vp]
    L.ppenv_step_into.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ppenv_step_sequence.argtypes = [vp, vp, i32, vp]
    L.ppenv_reset_all.argtypes = [vp, vp]
    L.ppenv_reduce_stats.argtypes = [vp, vp, vp]
    L.ppenv_reset_idx.argtypes = [vp, vp, i32, C.c_int, vp]
    L.ppenv_pd_targets.argtypes = [vp, vp, vp, vp]
    L.ppenv_serve_from_draws.argtypes = [vp, vp, i32, vp, vp]
    L.ppenv_set_randomization.argtypes = [vp, C.POINTER(scene.Randomization)]
    L.ppenv_set_gravity.argtypes = [vp, f32]
    L.ppenv_status.restype = C.c_uint32
    L.ppenv_status.argtypes = [vp]
    L.ppenv_step_kernel_name.restype = C.c_char_p
    L.ppenv_step_kernel_name.argtypes = [vp]
    L.ppenv_ta_sim_set_gravity.argtypes = [vp, f32, vp]
    L.ppenv_ta_sim_kernel_name.restype = C.c_char_p
    L.ppenv_ta_sim_kernel_name.argtypes = [vp]
    L.ppenv_ta_pd_targets.argtypes = [vp, i32, vp, vp, vp]
    L.ppenv_ta_serve_from_draws.argtypes = [vp, vp, i32, vp, vp]
    L.ppenv_ta_sim_device.argtypes = [vp]
    L.ppenv_ta_sim_status.restype = C.c_uint32
    L.ppenv_ta_sim_status.argtypes = [vp]
    L.ppenv_ta_sim_kernel.argtypes = [vp]
    L.ppenv_ta_sim_set_policy_input.argtypes = [vp, vp, vp, f32, vp, i32]
    L.ppenv_ta_sim_set_randomization.argtypes = [vp, C.POINTER(scene.Randomization)]
    L.ppenv_ta_model_is_compiled.argtypes = [cfgp, C.POINTER(scene.TAModel)]
    L.ppenv_post_physics_step.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    for name in ("ppenv_refresh_root_states", "ppenv_refresh_dof_states", "ppenv_refresh_dof_force",
                 "ppenv_refresh_rigid_body_states"):
        getattr(L, name).argtypes = [vp, vp, vp]
    L.ppenv_set_serve_override.argtypes = [vp, vp, C.c_int, vp]
    L.ppenv_ta_post_physics_step.argtypes = [C.POINTER(scene.TAParams)] + [vp] * 15
    L.ppenv_t4_rewards.argtypes = [C.POINTER(scene.T4Params)] + [vp] * 15
    L.ppenv_ta_sim_create.argtypes = [cfgp, C.POINTER(scene.TAModel), vp, C.POINTER(vp)]
    L.ppenv_ta_sim_destroy.restype = None
    L.ppenv_ta_sim_destroy.argtypes = [vp]
    L.ppenv_ta_simulate.argtypes = [vp, i32] + [vp] * 7
    L.ppenv_ta_forward_kinematics.argtypes = [vp, i32] + [vp] * 4
    L.ppenv_ta_step.argtypes = [vp, C.POINTER(scene.TAParams)] + [vp] * 16
    L.ppenv_state_bytes.restype = sz
    L.ppenv_state_bytes.argtypes = [vp]
    L.ppenv_get_state.argtypes = [vp, vp, sz]
    L.ppenv_set_state.argtypes = [vp, vp, sz]
    # ---- include/ppenv_dr.h
    L.ppenv_dr_state_bytes.restype = L.ppenv_dr_state_draws_offset.restype = sz
    L.ppenv_dr_state_bytes.argtypes = L.ppenv_dr_state_draws_offset.argtypes = [i32]
    L.ppenv_dr_plan_upload.argtypes = [C.POINTER(scene.DRPlan), vp, vp]
    L.ppenv_dr_apply.argtypes = [vp, i32, vp, vp, vp, vp]
    L.ppenv_dr_apply_ids.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    # ---- include/ppenv_policy.h
    L.ppenv_mlp_layer_forward.argtypes = [layerp, vp]
    L.ppenv_mlp_layer_forward_share.argtypes = [layerp, i32, vp]
    L.ppenv_mlp_chain_workspace_bytes.restype = sz
    L.ppenv_mlp_chain_workspace_bytes.argtypes = [i32, i32, i32]
    L.ppenv_mlp_chain_forward.argtypes = [layerp, i32, vp, vp]
    L.ppenv_mlp_chain_status.argtypes = [vp]
    L.ppenv_mlp_prepare_input.argtypes = [vp, i32, i32, i32, vp, vp, f32, vp, i32, vp]
    L.ppenv_mlp_sample_actions.argtypes = [vp, i32, i32, i32, vp, u64, u64, f32, f32, vp, vp, vp]
    L.ppenv_mlp_heads_sample.argtypes = [layerp, i32, vp, u64, u64, f32, f32, vp, vp, vp]
    L.ppenv_gae.argtypes = [vp, vp, i32, i64, vp, i32, i32, f32, f32, f32, vp, vp, vp]
    L.ppenv_mlp_layer_backward_input.argtypes = [layerp, vp, i64, i32, vp, i64, i32, vp]
    L.ppenv_mlp_dw_workspace_bytes.restype = sz
    L.ppenv_mlp_dw_workspace_bytes.argtypes = [C.POINTER(MLPDw)]
    L.ppenv_mlp_layer_backward_weight.argtypes = [C.POINTER(MLPDw), vp]
    L.ppenv_mlp_reduce_rows.argtypes = [vp, i32, i64, i64, vp, i32, vp]
    L.ppenv_mlp_bias_grad_workspace_bytes.restype = sz
    L.ppenv_mlp_bias_grad_workspace_bytes.argtypes = [i32, i32]
    L.ppenv_mlp_bias_grad_f32.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp]
    L.ppenv_mlp_cast_weights.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, i32, vp]
    L.ppenv_mlp_cast_weights_batch.argtypes = [C.POINTER(MLPCast), i32, vp]
    L.ppenv_running_mean_std_workspace_bytes.restype = sz
    L.ppenv_running_mean_std_workspace_bytes.argtypes = [i32, i32]
    L.ppenv_running_mean_std_update.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, f32, vp, vp]
    # ---- include/ppenv_ppo.h
    L.ppenv_ppo_loss_partial_floats.restype = sz
    L.ppenv_ppo_loss_partial_floats.argtypes = [i32]
    L.ppenv_ppo_loss_grad.argtypes = [C.POINTER(PPOLossArgs), vp]
    L.ppenv_ppo_grad_sumsq.argtypes = [vp, i32, vp, i32, vp]
    L.ppenv_ppo_adam_step.argtypes = [vp, i32, vp, i32, PPOAdam, vp, vp, vp, vp]
    # ---- include/ppenv_play.h
    L.ppenv_play_partial_bytes.restype = sz
    L.ppenv_play_partial_bytes.argtypes = [i32]
    L.ppenv_play_reset.argtypes = [i32, i32, vp, vp, vp, vp]
    L.ppenv_play_accumulate.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp, vp, vp]
    # ---- include/ppenv_play_group.h
    L.pp_play_group_partial_bytes.restype = sz
    L.pp_play_group_partial_bytes.argtypes = [i32, i32]
    L.pp_play_group_reset.argtypes = [i32, i32, i32, vp, vp, vp, vp]
    L.pp_play_group_accumulate.argtypes = [vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, vp]
    # ---- include/ppenv_play_pair.h
    L.pp_play_pair_ret_bytes.restype = L.pp_play_pair_len_bytes.restype = sz
    L.pp_play_pair_ret_bytes.argtypes = L.pp_play_pair_len_bytes.argtypes = [i32, i32, i32, i32]
    L.pp_play_pair_reset.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.pp_play_pair_record.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.pp_play_pair_reduce.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    # ---- include/ppenv_play_act.h
    L.pp_play_act_state_bytes.restype = L.pp_play_act_partial_bytes.restype = sz
    L.pp_play_act_state_bytes.argtypes = L.pp_play_act_partial_bytes.argtypes = [i32, i32, i32]
    L.pp_play_act_reset.argtypes = [i32, i32, i32, vp, vp, vp, vp]
    L.pp_play_act_accumulate.argtypes = [C.POINTER(PlayActInputs), vp, i32, i32, i32, i32, i64, vp, C.POINTER(PlayActThresholds), vp, vp, vp, vp, vp]
    # ---- include/ppenv_play_delay.h
    L.pp_play_delay_ring_bytes.restype = sz
    L.pp_play_delay_ring_bytes.argtypes = [i32, i32, i32]
    L.pp_play_delay_reset.argtypes = [i32, vp, vp]
    L.pp_play_delay_push.argtypes = [vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]
    # ---- include/ppenv_train_delay.h
    L.pp_train_delay_ring_bytes.restype = L.pp_train_delay_table_bytes.restype = sz
    L.pp_train_delay_ring_bytes.argtypes = [i32, i32, i32]
    L.pp_train_delay_table_bytes.argtypes = [i32]
    L.pp_train_delay_reset.argtypes = [i32, vp, vp, vp]
    L.pp_train_delay_push.argtypes = [vp, i64, vp, i32, i32, i32, C.POINTER(TrainDelayConsts), vp, vp, vp, vp, vp, i64, vp]
    # ---- include/ppenv_sensor.h
    L.pp_sensor_table_bytes.restype = L.pp_sensor_held_bytes.restype = sz
    L.pp_sensor_table_bytes.argtypes = [i32]
    L.pp_sensor_held_bytes.argtypes = [i32, i32]
    L.pp_sensor_reset.argtypes = [i32, vp, vp, vp]
    L.pp_sensor_push.argtypes = [vp, i64, vp, i32, i32, i32, C.POINTER(SensorConsts), vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    # ---- include/ppenv_ppo_meter.h
    L.ppo_meter_partial_bytes.restype = sz
    L.ppo_meter_partial_bytes.argtypes = [i32, i32]
    L.ppo_meter_update.argtypes = [vp, i64, vp, i64, i32, i32, i32, i64, vp, vp, vp, vp, vp]
    # ---- include/ppenv_render.h
    scenep = C.POINTER(RenderScene)
    L.pp_render_scene_upload.argtypes = [scenep, C.POINTER(RenderPrim), vp, vp]
    L.pp_render_pose.argtypes = [scenep, vp, vp, i32, vp, vp]
    L.pp_render_rays.argtypes = [scenep, C.POINTER(RenderCamera), vp, vp, i32, vp, vp, vp, vp]
    L.pp_render_rays_aa.argtypes = [scenep, C.POINTER(RenderCamera), vp, vp, i32, i32, vp, vp]
    L.pp_render_pose_anchor.argtypes = [scenep, vp, vp, i32, i32, i32, vp, vp, vp]
    L.pp_render_rays_frames.argtypes = [scenep, C.POINTER(RenderCamera), vp, vp, i32, i32, i32, vp, vp]
    # ---- include/ppenv_ta_outcome.h
    L.pp_ta_sim_set_outcome.argtypes = [vp, vp]
    L.pp_ta_post_physics_step_outcome.argtypes = [C.POINTER(scene.TAParams)] + [vp] * 16
    L.pp_ta_outcome_latch.argtypes = [vp, vp, i64, vp, vp]
    # ---- include/ppenv_serve.h
    L.pp_serve_plan_upload.argtypes = [C.POINTER(ServePlan), C.POINTER(ServeCell), vp, vp, vp]
    L.pp_serve_fill.argtypes = [vp, i32, vp, vp, vp]
    L.pp_serve_apply.argtypes = [vp, i32, vp, vp, vp, vp]
    L.pp_serve_apply_ids.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    # ---- include/ppenv_serve_curric.h
    statep = C.POINTER(ServeCurricState)
    L.pp_serve_curric_upload.argtypes = [C.POINTER(ServeCurric), C.POINTER(ServeCell), vp, vp, vp]
    L.pp_serve_curric_fill.argtypes = [vp, i32, i32, statep, vp, vp]
    L.pp_serve_curric_step.argtypes = [vp, i32, vp, vp, statep, vp, vp, vp, vp]
    L.pp_serve_curric_fold_bytes.restype = sz
    L.pp_serve_curric_fold_bytes.argtypes = [i64]
    L.pp_serve_curric_fold.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.pp_serve_curric_update.argtypes = [vp, i32, vp, statep, vp]
    # ---- include/ppenv_dr_adr.h
    adrsp = C.POINTER(AdrState)
    L.pp_dr_adr_upload.argtypes = [C.POINTER(Adr), C.c_double, vp, vp]
    L.pp_dr_adr_fill.argtypes = [vp, i32, i32, adrsp, vp]
    L.pp_dr_adr_step.argtypes = [vp, i32, vp, vp, adrsp, vp, vp, vp]
    L.pp_dr_adr_update.argtypes = [vp, i32, vp, adrsp, vp]
    # ---- include/ppenv_critic_input.h
    L.pp_critic_input_upload.argtypes = [C.POINTER(CriticTable), vp, vp]
    L.pp_critic_input_gather.argtypes = [vp, i32, i32, vp, i64, vp]
    L.pp_critic_input_prepare.argtypes = [vp, i64, i32, i32, vp, vp, f32, vp, i32, i32, vp]
    # ---- include/ppenv_history.h
    L.pp_history_width.restype = i32
    L.pp_history_width.argtypes = [i32, i32, i32, i32]
    L.pp_history_push.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, f32, f32, vp]
    return L


def stream(x):
    """The raw handle of torch's current stream on the device of `x` (a tensor or a device): what every launch's `stream` argument gets."""
    return torch.cuda.current_stream(getattr(x, "device", x)).cuda_stream


def ptr(t):
    """A tensor's device address, or None (a NULL pointer) for None."""
    return t.data_ptr() if t is not None else None


def check(rc, L=None):
    if rc != 0:
        raise PPEnvError(f"ppenv error {rc}: {(L if L is not None else lib()).ppenv_last_error().decode()}")
