"""The sensor flags of both command lines and the sweep's classification of the sensor axes, without a GPU: python -m isaacgym_amd.play
(--obs-noise S ... --action-drop-columns SPEC, fixed levels) and python -m isaacgym_amd.ppo (S or LO:HI, drawn per episode), what each
refuses before anything is built, and Sweep's four kinds of axes."""
import pytest

from isaacgym_amd import play, ppo, sensor
from isaacgym_amd.play import cli, sweep

TT, TA = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1"


def test_the_play_parser_takes_the_eight_flags():
    a = cli.parse_args(["--checkpoint", "x", "--task", TT, "--obs-noise", "0.01", "--obs-drop", "0.2", "--action-noise", "0.05", "--action-drop", "1",
                        "--obs-noise-columns", "ball_pos=1,ball_vel=4,60:67=0.5", "--obs-drop-columns", "ball_pos,ball_vel", "--action-noise-columns", "0:3=2",
                        "--action-drop-columns", "all"])
    assert (a.obs_noise, a.obs_drop, a.action_noise, a.action_drop) == (0.01, 0.2, 0.05, 1.0)
    assert (a.obs_noise_columns, a.obs_drop_columns, a.action_noise_columns, a.action_drop_columns) == ("ball_pos=1,ball_vel=4,60:67=0.5", "ball_pos,ball_vel", "0:3=2", "all")
    d = cli.parse_args(["--checkpoint", "x"])
    assert (d.obs_noise, d.obs_drop, d.action_noise, d.action_drop) == (0.0, 0.0, 0.0, 0.0) and d.obs_noise_columns is None and d.action_drop_columns is None
    a = cli.parse_args(["--checkpoint", "x", "--task", TT, "--sweep", "obs_noise=0:0.02:3", "--sweep", "obs_drop=0,0.5", "--paired"])
    sw = play.Sweep.parse(a.sweep, paired=a.paired)
    assert len(sw) == 6 and sw.cells[1] == {"obs_noise": 0.0, "obs_drop": 0.5} and sw.cells[4] == {"obs_noise": 0.02, "obs_drop": 0.0}


@pytest.mark.parametrize("argv, text", [
    (["--obs-noise", "-0.1"], "--obs-noise a noise amplitude is a finite number >= 0, not -0.1"),
    (["--action-noise", "nan"], "--action-noise a noise amplitude is a finite number >= 0"),
    (["--obs-drop", "1.5"], "--obs-drop a dropout probability is a number in 0..1, not 1.5"),
    (["--action-drop", "-1"], "--action-drop a dropout probability is a number in 0..1"),
    (["--task", TT, "--obs-noise-columns", "ball"], "--obs-noise-columns: 'ball': unknown column group 'ball'; the groups are all, body_pos, body_vel, dof_pos, dof_vel, "
                                                    "ball_pos, ball_vel, or a range LO:HI"),
    (["--task", TA, "--obs-drop-columns", "ball_pos"], "--obs-drop-columns: 'ball_pos': unknown column group 'ball_pos'; the groups are all, or a range LO:HI"),
    (["--task", TT, "--obs-noise-columns", "70:81"], "--obs-noise-columns: '70:81': the range 70:81 is not inside 0:80 with LO < HI"),
    (["--task", TT, "--action-noise-columns", "0:8"], "--action-noise-columns: '0:8': the range 0:8 is not inside 0:7"),
    (["--task", TA, "--action-drop-columns", "20:28"], "--action-drop-columns: '20:28': the range 20:28 is not inside 0:27"),
    (["--task", TT, "--action-noise-columns", "ball_pos"], "--action-noise-columns: 'ball_pos': unknown column group"),
    (["--task", TT, "--obs-drop-columns", "ball_pos=2"], "--obs-drop-columns: 'ball_pos=2': these columns take no scale"),
    (["--sweep", "obs_drop=0,1.5"], "sweep axis 'obs_drop': a dropout probability is a number in 0..1, not 1.5"),
    (["--sweep", "action_noise=-1,0"], "sweep axis 'action_noise': a noise amplitude is a finite number >= 0, not -1.0"),
    (["--sweep", "obs_noise[0]=1"], "an axis is one of"),
])
def test_the_play_parser_refuses(argv, text, capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(["--checkpoint", "x"] + argv)
    assert text in capsys.readouterr().err


def test_sweep_classifies_the_sensor_axes_once():
    assert play.SENSOR_AXES == sweep.SENSOR_AXES == sensor.AXES == ("obs_noise", "obs_drop", "action_noise", "action_drop")
    sw = play.Sweep([{"obs_noise": 0.01, "friction_scale": 0.5, "serve_speed": 5, "action_delay": 2}, {"action_drop": 1, "obs_drop": 0.25}, {}])
    assert sw.cell_sensors == [{"obs_noise": 0.01}, {"action_drop": 1.0, "obs_drop": 0.25}, {}] and sw.has_sensors and sw.has_latency
    assert sw.cell_latency == [{"action_delay": 2}, {}, {}] and [e[0] for e in sw.cell_tables[0]] == ["friction_scale"] and sw.cell_serves[0] == {"serve_speed": 5.0}
    assert all(type(v) is float for c in sw.cell_sensors for v in c.values()) and sw.cells[1] == {"action_drop": 1.0, "obs_drop": 0.25}
    assert sw.sensor_levels() == dict(obs_noise=[0.01, 0.0, 0.0], obs_drop=[0.0, 0.25, 0.0], action_noise=[0.0] * 3, action_drop=[0.0, 1.0, 0.0])
    assert sw.sensor_levels(obs_noise=0.5, action_drop=0.1)["obs_noise"] == [0.01, 0.5, 0.5] and sw.sensor_levels(action_drop=0.1)["action_drop"] == [0.1, 1.0, 0.1]
    assert sweep.cell_sensors([{}]) == dict(obs_noise=[0.0], obs_drop=[0.0], action_noise=[0.0], action_drop=[0.0])
    assert sweep.cell_sensors(sw.cell_sensors, 0.5, 0.5, 0.5, 0.5) == sw.sensor_levels(0.5, 0.5, 0.5, 0.5)
    # a sweep about the sensors alone leaves the physics and the serves alone
    only = play.Sweep([{"obs_noise": 0.0}, {"obs_noise": 0.02}])
    assert only.has_sensors and not only.sets_randomization and not only.needs_serve_plan and not only.has_latency
    assert only.tables({"friction_scale": 0}, 4) == {} and only.serve_cells({}) is None and only.cell_delays() == dict(action_delay=[0, 0], obs_delay=[0, 0])
    assert not play.Sweep([{}, {}]).has_sensors and play.Sweep([{}, {}]).sets_randomization
    assert play.cell_text(only.cells[1]) == "obs_noise=0.02"
    for axis, v in (("obs_noise", -1), ("obs_noise", float("inf")), ("obs_noise", (0, 1)), ("obs_noise", "1"), ("obs_noise", True), ("obs_noise", None),
                    ("action_drop", 1.01), ("action_drop", -0.01), ("obs_drop", float("nan")), ("obs_drop", [0.1, 0.2])):
        with pytest.raises(ValueError, match=f"sweep axis '{axis}': a "):
            play.Sweep([{axis: v}])
    with pytest.raises(ValueError, match="'obs_drop': a dropout probability"):
        sweep.cell_sensors([{}], obs_drop=2)
    assert play.sensor_line(dict(obs_noise=[0.0, 0.01], obs_drop=[0.5, 0.5], action_noise=[0.0, 0.0], action_drop=[0.0, 0.0],
                                 columns=dict(obs_noise_columns="ball_pos", obs_drop_columns=None))) == \
        "sensor: obs_noise 0,0.01; obs_drop 0.5,0.5; action_noise 0,0; action_drop 0,0; obs_noise_columns ball_pos"


@pytest.mark.parametrize("argv, text", [
    (["--obs-noise", "-1"], "--obs-noise: a number S or a range LO:HI"), (["--obs-noise", "0.2:0.1"], "--obs-noise: "), (["--action-noise", "inf"], "--action-noise: "),
    (["--obs-drop", "1.5"], "--obs-drop: a number S or a range LO:HI / \\(lo, hi\\) with 0 <= lo <= hi <= 1"), (["--action-drop", "0:2"], "--action-drop: "),
    (["--obs-noise", "x"], "--obs-noise: "), (["--task", TT, "--obs-noise-columns", "ball"], "--obs-noise-columns: 'ball': unknown column group 'ball'"),
    (["--task", TT, "--obs-drop-columns", "70:81"], "--obs-drop-columns: '70:81': the range 70:81 is not inside 0:80"),
    (["--task", TA, "--obs-noise-columns", "ball_pos"], "--obs-noise-columns: 'ball_pos': unknown column group"),
    (["--task", TT, "--action-drop-columns", "0:8"], "--action-drop-columns: '0:8': the range 0:8 is not inside 0:7"),
])
def test_the_trainer_cli_refuses_before_anything_is_built(argv, text):
    with pytest.raises(ValueError, match=text):
        ppo.main(argv)


def test_the_trainer_takes_numbers_ranges_and_text():
    assert sensor.sigma_range("--obs-noise", "0:0.02") == (0.0, 0.02) and sensor.drop_range("--obs-drop", "0.2") == (0.2, 0.2)
    assert sensor.sensor_text(dict(obs_noise=[0.0, 0.02], obs_drop=[0.2, 0.2], action_noise=[0.0, 0.0], action_drop=[0.0, 0.0],
                                   columns=dict(obs_noise_columns="ball_pos", obs_drop_columns=None, action_noise_columns=None, action_drop_columns=None))) == \
        "sensor: obs_noise 0..0.02, drawn per episode; obs_drop 0.2; action_noise 0; action_drop 0; obs_noise_columns ball_pos"
    sensor.check_specs(TT, dict(obs_noise_columns="ball_pos=1,ball_vel=4,60:67=0.5", obs_drop_columns="ball_pos", action_noise_columns="0:7", action_drop_columns=None))
    sensor.check_specs("no such task", dict(obs_noise_columns="whatever"))                   # left to make()
