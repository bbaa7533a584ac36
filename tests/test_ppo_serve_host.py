"""What PPOTrainer(serve_plan=, curriculum=), curriculum.ServeCurriculum and the trainer's CLI refuse before anything touches the device, and
how the CLI's --serve / --curriculum flags parse.  No GPU."""
import math
import types

import pytest

from isaacgym_amd import _lib, curriculum, ppo, scene, serve


class Handle:
    """An env handle as far as ServeCurriculum looks at it before its first device allocation."""
    L, device, num_envs, num_agents = None, "cuda:0", 8, 1

    def serve_defaults(self):
        return {"serve_speed": (8.0, 8.6), "serve_tilt": (-5.0, 5.0), "serve_tilt_z": (2.0, 10.0)}

    def serve_target(self):
        return dict(axes=serve.AXES_7DOF, out=None, form=scene.VARIANT_TT, layout=_lib.SERVE_LAYOUT_SOA3, reset_rows=1, seed=1, env_id_offset=0)


BINS = curriculum.grid({"serve_speed": (6.0, 9.0, 2)})


def test_plan_together_with_curriculum_is_refused():
    task = types.SimpleNamespace(randomize=False, _serve_plan=None)
    with pytest.raises(ValueError, match="serve_plan together with curriculum"):
        ppo.PPOTrainer(task, ppo.PPOConfig(), serve_plan=[{}], curriculum=dict(bins=BINS))
    for kw in (dict(serve_plan=[{}]), dict(curriculum=dict(bins=BINS))):                       # a task with a plan of its own is refused whatever is asked
        with pytest.raises(ValueError, match="clear_serve_plan"):
            ppo.PPOTrainer(types.SimpleNamespace(randomize=False, _serve_plan=object()), ppo.PPOConfig(), **kw)


@pytest.mark.parametrize("kw, text", [(dict(power=-1), "power"), (dict(power=5), "power"), (dict(power=1.5), "power"), (dict(power=True), "power"),
                                      (dict(mix=-0.1), "mix"), (dict(mix=1.1), "mix"), (dict(mix=math.nan), "mix"), (dict(mix="x"), "mix"),
                                      (dict(alpha=0.0), "alpha"), (dict(alpha=1.01), "alpha"), (dict(alpha=math.inf), "alpha")])
def test_parameters_out_of_range(kw, text):
    with pytest.raises(ValueError, match=f"curriculum {text}"):
        curriculum.ServeCurriculum(Handle(), BINS, **kw)
    with pytest.raises(ValueError, match=f"curriculum {text}"):
        curriculum.check_parameters(**dict(dict(power=1, mix=0.25, alpha=0.3), **kw))
    assert curriculum.check_parameters(0, 0, 1) == (0, 0.0, 1.0) and curriculum.check_parameters(4, 1.0, 0.01) == (4, 1.0, 0.01)


def test_bins_and_axes():
    with pytest.raises(ValueError, match="257 bins"):
        curriculum.ServeCurriculum(Handle(), [{}] * 257)
    with pytest.raises(ValueError, match="0 bins"):
        curriculum.ServeCurriculum(Handle(), [])
    with pytest.raises(ValueError, match="289 bins"):
        curriculum.grid({"serve_speed": (6, 9, 17), "serve_tilt": (-5, 5, 17)})
    with pytest.raises(ValueError, match="serve axis 'ball_y': this environment's serve axes are serve_speed, serve_tilt, serve_tilt_z"):
        curriculum.ServeCurriculum(Handle(), curriculum.grid({"ball_y": (-0.3, 0.0, 2)}))
    with pytest.raises(ValueError, match="serve axis 'spin'"):
        curriculum.ServeCurriculum(Handle(), [{"spin": 1.0}])
    with pytest.raises(ValueError, match="beyond \\+-57 degrees"):
        curriculum.ServeCurriculum(Handle(), [{"serve_tilt": (-58.0, 0.0)}])


def test_serve_flags_parse_to_one_cell():
    assert ppo.serve_cell_parse([]) is None and ppo.serve_cell_parse(None) is None
    cells = ppo.serve_cell_parse(["serve_speed=7.5", "serve_tilt=-3:4"])
    assert cells == [{"serve_speed": "7.5", "serve_tilt": ("-3", "4")}]
    assert serve.resolve_cells(cells, Handle().serve_defaults(), serve.AXES_7DOF) == [{"serve_speed": (7.5, 7.5), "serve_tilt": (-3.0, 4.0), "serve_tilt_z": (2.0, 10.0)}]
    with pytest.raises(ValueError, match="expected AXIS=V or AXIS=LO:HI"):
        ppo.serve_cell_parse(["serve_speed"])
    for bad in (["serve_speed=fast"], ["serve_speed=9:6"], ["serve_speed=1:2:3"]):              # serve.value_range's own text
        with pytest.raises(ValueError, match="is not a finite number or a \\(lo, hi\\) pair"):
            serve.resolve_cells(ppo.serve_cell_parse(bad), Handle().serve_defaults(), serve.AXES_7DOF)
    with pytest.raises(ValueError, match="this environment's serve axes are"):
        serve.resolve_cells(ppo.serve_cell_parse(["ball_y=0"]), Handle().serve_defaults(), serve.AXES_7DOF)


@pytest.mark.parametrize("argv, text", [(["--serve", "serve_speed=7", "--curriculum", "serve_speed=6:9:2"], "--serve together with --curriculum"),
                                        (["--curriculum", "serve_speed=6:9"], "expected AXIS=LO:HI:BINS"),
                                        (["--curriculum", "serve_speed=6:9:300"], "300 bins"),
                                        (["--curriculum", "serve_speed=6:9:2", "--curriculum-power", "5"], "curriculum power"),
                                        (["--curriculum", "serve_speed=6:9:2", "--curriculum-mix", "1.5"], "curriculum mix"),
                                        (["--curriculum", "serve_speed=6:9:2", "--curriculum-alpha", "0"], "curriculum alpha"),
                                        (["--serve", "serve_speed"], "expected AXIS=V or AXIS=LO:HI")])
def test_cli_refuses_before_it_builds_anything(capsys, argv, text):
    with pytest.raises(SystemExit) as e:
        ppo.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_table_lines():
    table = dict(epoch=3, power=1, mix=0.25, alpha=0.3, bins=[dict(bin=0, cell={"serve_speed": [6.0, 7.5]}, games=4, mean_return=-1.25, dropped=0, prob=0.75),
                                                              dict(bin=1, cell={"serve_speed": [7.5, 9.0]}, games=0, mean_return=0.0, dropped=2, prob=0.25)])
    assert curriculum.table_lines(table) == ["serve curriculum at epoch 3: 2 bins", "  bin 0: cell serve_speed=6..7.5  games 4  mean return -1.25  prob 0.7500",
                                             "  bin 1: cell serve_speed=7.5..9  games 0  mean return -  prob 0.2500  dropped 2"]
