"""Privileged critic inputs, the part that needs no GPU (isaacgym_amd.critic_input; include/ppenv_critic_input.h): name resolution and
every refusal by its message, column order and P for each task's DR_TABLE_ROWS, the checkpoint record and its check, the checkpoint
reader with a wider critic, the C entry points' refusals before any device call — and the numpy restatement the GPU tests compare the
kernels against (critic_input_reference), checked here against hand-written cases."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import critic_input_reference as ref
from isaacgym_amd import _lib, critic_input as ci, dr
from isaacgym_amd.env import PPEnv
from isaacgym_amd.tensor_api import TAEnv


def fake_env(table_rows, names, n=6):
    if names is None:
        return types.SimpleNamespace(dr_tables=None)
    return types.SimpleNamespace(dr_tables=[torch.zeros((table_rows[k], n) if table_rows[k] else (n,)) if k in names else None for k in dr.TABLE_NAMES])


def fake_lines(rows=6, num_obs=80, act=True, obs=True):
    line = lambda: types.SimpleNamespace(delays=torch.zeros(rows, dtype=torch.int32))
    return types.SimpleNamespace(act_line=line() if act else None, obs_line=line() if obs else None,
                                 raw_obs=torch.zeros(rows, num_obs + 7)[:, :num_obs] if obs else None)


# ------------------------------------------------------------------------------------------------------ names and refusals
def test_names_are_parsed_in_the_given_order_and_unknown_or_repeated_ones_are_refused():
    assert ci.parse(()) == ci.parse(None) == ci.parse("") == ()
    assert ci.parse("tables,latency,raw_obs") == ci.parse(["tables", "latency", "raw_obs"]) == ("tables", "latency", "raw_obs")
    assert ci.parse(" raw_obs , tables ") == ("raw_obs", "tables")
    with pytest.raises(ValueError, match="critic_inputs: 'masses' is not one of tables, latency, raw_obs"):
        ci.parse("tables,masses")
    with pytest.raises(ValueError, match="critic_inputs: a name is given twice"):
        ci.parse(("tables", "tables"))


def test_every_refusal_names_the_argument_and_says_what_is_missing():
    rows = PPEnv.DR_TABLE_ROWS
    with pytest.raises(ValueError, match="critic_inputs: 'tables' needs a run with randomisation"):
        ci.resolve(types.SimpleNamespace(dr_tables=None), fake_lines(), ("tables",))
    with pytest.raises(ValueError, match="critic_inputs: 'tables' needs a run with randomisation"):
        ci.resolve(fake_env(rows, ()), fake_lines(), ("tables",))                               # tables set, every one None
    with pytest.raises(ValueError, match="critic_inputs: 'latency' needs a delay line"):
        ci.resolve(fake_env(rows, ("friction_scale",)), fake_lines(act=False, obs=False), ("tables", "latency"))
    with pytest.raises(ValueError, match="critic_inputs: 'raw_obs' needs an obs_delay line"):
        ci.resolve(fake_env(rows, None), fake_lines(obs=False), ("latency", "raw_obs"))
    with pytest.raises(ValueError, match="critic_inputs: 'raw_obs' needs an obs_delay line"):
        ci.columns(("raw_obs",), rows, None, (0, 2), (0, 0), 80)
    with pytest.raises(ValueError, match="float32 or int32"):
        ci.source("tables", "friction_scale", torch.zeros(4, dtype=torch.float64), True)
    with pytest.raises(ValueError, match="at most 16 sources and 1024 columns"):
        ci.resolve(fake_env(rows, None), fake_lines(num_obs=1100), ("raw_obs",))


# ------------------------------------------------------------------------------------------------------ column order and P
@pytest.mark.parametrize("table_rows, want", [(PPEnv.DR_TABLE_ROWS, [7, 7, 7, 1, 1]), (TAEnv.DR_TABLE_ROWS, [27, 27, 28, 1, 1])], ids=["7dof", "27dof"])
def test_tables_come_in_table_names_order_one_column_per_table_row(table_rows, want):
    assert tuple(table_rows) == dr.TABLE_NAMES
    src = ci.resolve(fake_env(table_rows, dr.TABLE_NAMES), fake_lines(), ("tables",))
    assert [s.label for s in src] == list(dr.TABLE_NAMES) and [s.cols for s in src] == want
    assert all(s.table_major and s.stride == 6 and s.kind == _lib.CRITIC_F32 for s in src)
    assert ci.record(src) == {"names": ["tables"], "columns": [sum(want)], "P": sum(want)}
    # only the tables that are set, still in TABLE_NAMES order
    some = ci.resolve(fake_env(table_rows, ("friction_scale", "link_mass_scale")), fake_lines(), ("tables",))
    assert [s.label for s in some] == ["link_mass_scale", "friction_scale"] and [s.cols for s in some] == [want[2], 1]


def test_sources_follow_the_names_and_the_record_counts_columns_per_name():
    env = fake_env(PPEnv.DR_TABLE_ROWS, ("dof_damping_scale", "restitution_scale"))
    src = ci.resolve(env, fake_lines(num_obs=80), ("raw_obs", "latency", "tables"))
    assert [s.label for s in src] == ["raw_obs", "action_delay", "obs_delay", "dof_damping_scale", "restitution_scale"]
    assert [(s.cols, s.table_major, s.stride, s.kind) for s in src] == [(80, False, 87, 0), (1, False, 1, 1), (1, False, 1, 1), (7, True, 6, 0), (1, True, 6, 0)]
    rec = ci.record(src)
    assert rec == {"names": ["raw_obs", "latency", "tables"], "columns": [80, 2, 8], "P": 90}
    assert [s.label for s in ci.resolve(env, fake_lines(act=False), ("latency",))] == ["obs_delay"]          # the lines that exist
    # what the trainer computes before the collector exists is the same record
    assert ci.columns(("raw_obs", "latency", "tables"), PPEnv.DR_TABLE_ROWS, ["dof_damping_scale", "restitution_scale"], (0, 2), (1, 1), 80) == rec
    assert ci.columns(("latency",), PPEnv.DR_TABLE_ROWS, None, (0, 3), (0, 0), 80) == {"names": ["latency"], "columns": [1], "P": 1}
    full = ci.columns(("tables", "latency", "raw_obs"), PPEnv.DR_TABLE_ROWS, list(dr.TABLE_NAMES), (0, 3), (1, 1), 313)
    assert full["columns"] == [23, 2, 313] and full["P"] == 338
    assert ci.text({"names": ["tables", "latency", "raw_obs"], "columns": [30, 2, 313], "P": 345}, 313) == \
        "critic inputs: tables 30 + latency 2 + raw_obs 313 = 345 columns (first layer K 320 -> 704)"


# ------------------------------------------------------------------------------------------------------ the checkpoint record
def test_record_round_trips_through_torch_save_and_a_mismatch_is_refused_by_name(tmp_path):
    rec = {"names": ["tables", "latency"], "columns": [23, 2], "P": 25}
    path = tmp_path / "ck.pth"
    torch.save({"critic_inputs": rec, "epoch": 3}, path)
    back = torch.load(path, weights_only=True)["critic_inputs"]
    assert back == rec
    ci.check_record(back, rec)
    ci.check_record(None, None)                                                                  # a file and a trainer without: as before
    with pytest.raises(ValueError, match=r"trained with P = 25 privileged columns \(\['tables', 'latency'\]\), this trainer has P = 24"):
        ci.check_record(back, {"names": ["tables", "latency"], "columns": [23, 1], "P": 24})
    with pytest.raises(ValueError, match="trained with P = 25 .* this trainer has P = 0"):
        ci.check_record(back, None)
    with pytest.raises(ValueError, match="trained with P = 0 .* this trainer has P = 25"):
        ci.check_record(None, rec)
    with pytest.raises(ValueError, match="the checkpoint's names .* are not this trainer's"):
        ci.check_record(back, {"names": ["latency", "tables"], "columns": [2, 23], "P": 25})
    with pytest.raises(ValueError, match="are not this trainer's"):
        ci.check_record(back, {"names": ["tables", "latency"], "columns": [24, 1], "P": 25})


def test_checkpoint_reader_accepts_a_wider_critic_and_rejects_a_wider_actor():
    from isaacgym_amd.policy import layers_from_rlgames_state_dict, rlgames_state_dict_from_layers
    gen = torch.Generator().manual_seed(1)
    mlp = lambda d, out: [(torch.randn(16, d, generator=gen), torch.randn(16, generator=gen)), (torch.randn(out, 16, generator=gen), torch.randn(out, generator=gen))]
    sd = rlgames_state_dict_from_layers(mlp(10, 3), mlp(15, 1))
    actor, critic = layers_from_rlgames_state_dict(sd)
    assert actor[0][0].shape == (16, 10) and critic[0][0].shape == (16, 15)
    same = layers_from_rlgames_state_dict(rlgames_state_dict_from_layers(mlp(10, 3), mlp(10, 1)))
    assert same[0][0][0].shape == same[1][0][0].shape == (16, 10)                               # equal widths: as before
    with pytest.raises(ValueError, match="only the critic's first layer may be the wider one"):
        layers_from_rlgames_state_dict(rlgames_state_dict_from_layers(mlp(15, 3), mlp(10, 1)))


# ------------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_refuse_bad_arguments_before_any_device_call():
    L = _lib.lib()
    err = lambda: L.ppenv_last_error().decode()
    assert C.sizeof(_lib.CriticSource) == 32 and C.sizeof(_lib.CriticTable) == 16 + 16 * 32
    assert L.pp_critic_input_upload(None, 4096, None) == -1 and "NULL pointer" in err()
    t = _lib.CriticTable(rows=6, num_agents=3, sources=1)
    assert L.pp_critic_input_upload(C.byref(t), 4096, None) == -1 and "num_agents not 1 or 2" in err()
    t.num_agents, t.rows = 2, 5
    assert L.pp_critic_input_upload(C.byref(t), 4096, None) == -1 and "rows < 1 or no multiple of num_agents" in err()
    t.rows, t.sources = 6, 17
    assert L.pp_critic_input_upload(C.byref(t), 4096, None) == -1 and "sources outside 1 .. 16" in err()
    t.sources = 2
    t.source[0] = _lib.CriticSource(4096, 0, 4, 0, 0, 4)
    cases = [(_lib.CriticSource(0, 0, 4, 0, 0, 4), "source 1: a NULL pointer"), (_lib.CriticSource(4096, 2, 4, 0, 0, 4), "source 1: kind"),
             (_lib.CriticSource(4096, 0, 4, 2, 0, 4), "source 1: layout"), (_lib.CriticSource(4096, 0, 0, 0, 0, 4), "source 1: cols outside"),
             (_lib.CriticSource(4096, 0, 4, 0, 0, 3), "source 1: a stride below"), (_lib.CriticSource(4096, 0, 4, 1, 0, 2), "source 1: a stride below"),
             (_lib.CriticSource(4096, 0, 1021, 0, 0, 1021), "more than 1024 columns in all")]
    for src, text in cases:
        t.source[1] = src
        assert L.pp_critic_input_upload(C.byref(t), 4096, None) == -1 and text in err(), text
    assert L.pp_critic_input_gather(None, 6, 2, 4096, 8, None) == -1 and "pp_critic_input_gather" in err()
    assert L.pp_critic_input_gather(4096, 5, 2, 4096, 8, None) == -1
    assert L.pp_critic_input_gather(4096, 6, 3, 4096, 8, None) == -1
    ok = dict(priv=4096, ld_priv=7, rows=4, P=7, mean=None, inv_std=None, clip=5.0, x16=4096, ld_x16=384, col0=313, stream=None)
    for bad in (dict(priv=None), dict(x16=None), dict(rows=0), dict(P=0), dict(P=1025), dict(ld_priv=6), dict(col0=-1), dict(ld_x16=383), dict(col0=378),
                dict(x16=4104), dict(mean=4096)):
        assert L.pp_critic_input_prepare(*{**ok, **bad}.values()) == -1 and "pp_critic_input_prepare" in err(), bad


# ------------------------------------------------------------------------------------------------------ the numpy restatement
def test_numpy_gather_on_a_hand_written_case():
    table = np.array([[1, 2, 3], [4, 5, 6]], np.float32)                                        # [2 table rows, 3 envs]
    scalar = np.array([-0.0, 7, 8], np.float32)
    delays = np.array([0, 1, 2, 3, 4, 5], np.int32)
    wide = np.arange(24, dtype=np.float32).reshape(6, 4)
    src = [dict(array=table, table_major=True), dict(array=scalar, table_major=True), dict(array=delays, table_major=False),
           dict(array=wide[:, :3], table_major=False)]
    out = ref.gather(src, 6, 2)                                                                 # two actor rows per env
    assert out.shape == (6, 7)
    assert out[:, 0].tolist() == [1, 1, 2, 2, 3, 3] and out[:, 1].tolist() == [4, 4, 5, 5, 6, 6]
    assert out[:, 2].tolist() == [0, 0, 7, 7, 8, 8] and np.signbit(out[:2, 2]).all()            # the negative zero keeps its sign
    assert out[:, 3].tolist() == [0, 1, 2, 3, 4, 5] and np.array_equal(out[:, 4:], wide[:, :3])
    one = ref.gather(src[:2], 3, 1)
    assert np.array_equal(one, np.array([[1, 4, -0.0], [2, 5, 7], [3, 6, 8]], np.float32))
    assert ref.gather([dict(array=np.array([2 ** 24 + 1, -(2 ** 24 + 3)], np.int32), table_major=False)], 2, 1).ravel().tolist() == [2.0 ** 24, -(2.0 ** 24 + 4)]


def test_numpy_prepare_on_a_hand_written_case():
    x16 = np.full((2, 16), 9, np.float16)
    priv = np.array([[1.0, 100.0, -0.0], [3.0, -100.0, 2049.0]], np.float32)
    ref.prepare(x16, priv, np.array([1, 0, 0], np.float32), np.array([2, 1, 1], np.float32), 5.0, 5)
    assert (x16[:, :5] == 9).all() and (x16[:, 8:] == 0).all()
    assert x16[:, 5:8].tolist() == [[0, 5, 0], [4, -5, 5]] and np.signbit(x16[0, 7])
    ref.prepare(x16, priv, None, None, 5.0, 5)                                                  # converted only: 2049 rounds to even
    assert x16[:, 5:8].tolist() == [[1, 100, 0], [3, -100, 2048]]
