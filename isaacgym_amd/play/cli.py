"""python -m isaacgym_amd.play: the options, the checkpoints x cells of --against, the printed report and its JSON files."""
import argparse
import json

from .accounting import ACT_THRESHOLDS, DELAY_MAX
from .player import Player
from .report import actuator_table, cell_text, group_line, latency_line, outcome_lines, pair_line, sensor_line
from .sweep import SENSOR_AXES, Sweep, sensor_level


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m isaacgym_amd.play", description="play a checkpoint (rl_games' player) on the native env and network")
    ap.add_argument("--task", default="HumanoidPingpongTiltNESSparse27DOFG1")
    ap.add_argument("--checkpoint", required=True, help="nn/<task>.pth as python -m isaacgym_amd.ppo (or rl_games) writes it")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--games", type=int, default=2000, help="rl_games' games_num")
    ap.add_argument("--stochastic", action="store_true", help="draw the actions from Normal(mu, sigma) instead of playing mu")
    ap.add_argument("--sigma", type=float, default=None, help="override the log-std with this value (train.py:214); sigma = exp(value)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--cfg-dir", default=None, help="a reference cfg/ directory to compose the task yaml from")
    ap.add_argument("--poll-every", type=int, default=64, help="control steps between two host reads of the totals")
    ap.add_argument("--max-steps", type=int, default=108000)
    ap.add_argument("--outcomes", action="store_true", help="27-dof task: print the reference's five outcome counts (TA:1164-1168) as rates of the envs")
    ap.add_argument("--sweep", action="append", default=None, metavar="AXIS=SPEC", help="play under a grid of physical-parameter scales in one pass (repeatable: "
                    "one axis each; the envs are split into one group per cell and --games is per cell): AXIS is dof_stiffness_scale, dof_damping_scale, "
                    "link_mass_scale, restitution_scale or friction_scale, or one row of a table as NAME[ROW], or a serve axis: serve_speed, serve_tilt, "
                    "serve_tilt_z (degrees; may be negative), ball_y, ball_z (27-dof task), or a latency axis in whole control steps (0..15): action_delay, "
                    "obs_delay, or a sensor axis: obs_noise, action_noise (an amplitude >= 0), obs_drop, action_drop (a probability 0..1); SPEC is lo:hi:count "
                    "(inclusive) or v0,v1,...")
    ap.add_argument("--paired", action="store_true", help="with --sweep: env i of every cell is served the same sequence of balls (common random numbers), "
                    "so the serve noise cancels in the difference of two cells")
    ap.add_argument("--sweep-out", default=None, metavar="FILE.json", help="with --sweep: write the per-cell results (the result's `groups`) to FILE.json")
    ap.add_argument("--paired-diff", action="store_true", help="with --sweep ... --paired: per cell, the mean of return(cell) - return(baseline cell) over the "
                    "same balls (env i, episode m of both cells), with its own standard error")
    ap.add_argument("--baseline", type=int, default=None, metavar="INDEX", help="with --paired-diff: the baseline cell, in the order the cells are printed (default 0)")
    ap.add_argument("--paired-out", default=None, metavar="FILE.json", help="with --paired-diff or --against: write the result's `paired_diff` to FILE.json")
    ap.add_argument("--against", action="append", default=None, metavar="PATH", help="another checkpoint to play on the same balls (repeatable): the cells become "
                    "checkpoints x sweep cells, --checkpoint's first (without --sweep: one cell per checkpoint); implies --paired and --paired-diff, the "
                    "baseline of every cell being the same sweep cell under --checkpoint; --num-envs must be a multiple of the cell count")
    ap.add_argument("--actuators", action="store_true", help="per joint and per cell: torque against the effort limit, speed against the velocity limit, "
                    "position against the joint limits, mechanical energy per game and raw actions at clipActions, summed on the device; one table per cell")
    ap.add_argument("--actuators-out", default=None, metavar="FILE.json", help="with --actuators: write the result's `actuators` to FILE.json")
    ap.add_argument("--effort-frac", type=float, default=None, help=f"with --actuators: at the effort limit means |tau| >= this x effort (default {ACT_THRESHOLDS['effort_frac']})")
    ap.add_argument("--vel-frac", type=float, default=None, help=f"with --actuators: at the velocity limit means |qd| >= this x the limit (default {ACT_THRESHOLDS['vel_frac']})")
    ap.add_argument("--limit-margin", type=float, default=None, help="with --actuators: at a position limit means within this many rad of it, or beyond "
                    f"(default {ACT_THRESHOLDS['limit_margin']})")
    ap.add_argument("--action-delay", type=int, default=0, metavar="K", help=f"control latency of the command path: the env consumes the action of K control steps "
                    f"ago (0..{DELAY_MAX}; the episode's first action is held until there is one that old); with --sweep, the value of the cells that do not "
                    "name action_delay")
    ap.add_argument("--obs-delay", type=int, default=0, metavar="K", help=f"control latency of the sensing path: the policy sees the observation of K control "
                    f"steps ago (0..{DELAY_MAX}); with --sweep, the value of the cells that do not name obs_delay")
    for path, what in (("obs", "the observations the policy sees (before --obs-delay)"), ("action", "the commands the env consumes (after --action-delay)")):
        ap.add_argument(f"--{path}-noise", type=float, default=0.0, metavar="S", help=f"Gaussian noise of amplitude S x the column's scale on {what}, drawn on the "
                        f"device per env, episode and step; with --sweep, the value of the cells that do not name {path}_noise")
        ap.add_argument(f"--{path}-drop", type=float, default=0.0, metavar="P", help=f"each control step, with probability P (0..1), {what} are the last delivered "
                        f"ones again in the hold columns (never an episode's first sample); with --sweep, the value of the cells that do not name {path}_drop")
        ap.add_argument(f"--{path}-noise-columns", default=None, metavar="SPEC", help=f"the noised columns and their scales: comma-separated NAME[=SCALE] or "
                        "LO:HI[=SCALE] (HI exclusive), e.g. ball_pos=1,ball_vel=4,60:67=0.5; NAME is all" +
                        (", body_pos, body_vel, dof_pos, dof_vel, ball_pos, ball_vel (7-dof and 4-actor tasks)" if path == "obs" else "") + "; default all=1")
        ap.add_argument(f"--{path}-drop-columns", default=None, metavar="SPEC", help="the columns a dropout holds: comma-separated NAME or LO:HI; default all")
    ap.add_argument("--capture", default=None, metavar="FILE", help="record the run to FILE: .gif, .png (numbered files) or .npy (isaacgym_amd.render)")
    ap.add_argument("--capture-envs", default="0", help="comma-separated env ids to draw, side by side (at most 16)")
    ap.add_argument("--capture-len", type=int, default=300, help="frames kept: the last this many")
    ap.add_argument("--capture-every", type=int, default=2, help="control steps between two frames")
    ap.add_argument("--capture-size", default="640x480", help="WIDTHxHEIGHT of one env's picture")
    ap.add_argument("--capture-fps", type=float, default=30.0)
    ap.add_argument("--capture-samples", type=int, default=1, choices=(1, 2, 4), help="rays per pixel and axis: 2 is 2 x 2 supersampling, 4 is 4 x 4")
    ap.add_argument("--capture-deferred", action="store_true", help="record the posed primitives while playing and cast all rays in one batched launch at the "
                    "end (render.Trajectory): the same file, byte for byte")
    ap.add_argument("--capture-trajectory", default=None, metavar="FILE.npz", help="also save the recording as data (records deferred): "
                    "python -m isaacgym_amd.render replay draws it again at any size, sample count and camera")
    ap.add_argument("--camera", choices=("side", "follow"), default="side", help="side: table and humanoid(s); follow: the reference viewer's follow-cam")
    args = ap.parse_args(argv)
    if args.sweep_out and not args.sweep:
        ap.error("--sweep-out needs --sweep")
    if args.paired and not args.sweep:
        ap.error("--paired needs --sweep")
    if not args.actuators:
        for flag, v in (("--actuators-out", args.actuators_out), ("--effort-frac", args.effort_frac), ("--vel-frac", args.vel_frac),
                        ("--limit-margin", args.limit_margin)):
            if v is not None:
                ap.error(f"{flag} needs --actuators")
    if args.against:
        if args.baseline is not None:
            ap.error("--baseline does not go with --against: the baseline of every cell is the same sweep cell under --checkpoint")
        if args.outcomes:
            ap.error("--against plays the checkpoints as the cells of a sweep, and --outcomes cannot be split by cell")
    else:
        if args.paired_diff and not (args.sweep and args.paired):
            ap.error("--paired-diff needs --sweep ... --paired: without common serves, episode m of env i is a different ball in every cell")
        if args.baseline is not None and not args.paired_diff:
            ap.error("--baseline needs --paired-diff")
        if args.paired_out and not args.paired_diff:
            ap.error("--paired-out needs --paired-diff or --against")
    for flag, axis in (("--action-delay", "action_delay"), ("--obs-delay", "obs_delay")):
        if not 0 <= getattr(args, axis) <= DELAY_MAX:
            ap.error(f"{flag} is a number of whole control steps 0..{DELAY_MAX}")
    for axis in SENSOR_AXES:
        try:
            sensor_level(axis, getattr(args, axis))
        except ValueError as e:
            ap.error("--" + axis.replace("_", "-") + str(e).split(":", 1)[1])
    try:
        from .. import sensor
        sensor.check_specs(args.task, {f"{a}_columns": getattr(args, f"{a}_columns") for a in SENSOR_AXES}, flag=lambda key: "--" + key.replace("_", "-"))
    except ValueError as e:
        ap.error(str(e))
    if args.sweep:
        try:
            Sweep.parse(args.sweep)
        except ValueError as e:
            ap.error(str(e))
    return args


def actuator_option(args):
    """Player's `actuators` from the --actuators, --effort-frac, --vel-frac and --limit-margin options: False, True, or the dict of the
    thresholds that were given."""
    if not getattr(args, "actuators", False):
        return False
    given = {k: getattr(args, k, None) for k in ACT_THRESHOLDS}
    return {k: v for k, v in given.items() if v is not None} or True


def make_renderer(task, args):
    """The Renderer of the --capture-envs, --capture-size, --capture-samples (default 1) and --camera options.  (`args` may be another
    CLI's namespace — the trainer's — that has only some of the options: hence the getattr defaults here and in make_recorder.)"""
    from .. import render
    try:
        width, height = (int(v) for v in args.capture_size.lower().split("x"))
        envs = [int(v) for v in args.capture_envs.split(",")]
    except ValueError as e:
        raise SystemExit(f"--capture-size is WIDTHxHEIGHT and --capture-envs a comma-separated list of env ids: {e}")
    renderer = render.Renderer(task, envs=envs, width=width, height=height, samples=getattr(args, "capture_samples", 1))
    if args.camera == "follow":
        renderer.set_camera(render.Camera.follow_root(renderer.scene))
    return renderer


def make_recorder(task, args):
    """The Recorder of the --capture* options."""
    from .. import render
    deferred = bool(getattr(args, "capture_deferred", False) or getattr(args, "capture_trajectory", None))
    return render.Recorder(make_renderer(task, args), length=args.capture_len, every=args.capture_every, deferred=deferred)


def against_cells(args, task, policy, sweep):
    """--against: checkpoints x sweep cells, checkpoint-major, cell (k, c) against (0, c) -> (one policy per cell, the paired Sweep of all
    the cells, one baseline per cell).  Prints the checkpoints' numbers."""
    from ..policy import RLGamesPolicy
    cells = sweep.cells if sweep is not None else [{}]
    nets = [policy] + [RLGamesPolicy.load(p, task.device) for p in args.against]
    out = [net for net in nets for _ in cells], Sweep(cells * len(nets), paired=True), [c for _ in nets for c in range(len(cells))]
    for k, p in enumerate([args.checkpoint] + list(args.against)):
        print(f"checkpoint {k}: {p}", flush=True)
    return out


def print_report(args, task, res, recorder):
    """Everything main prints after the run, in order, and the --actuators-out, --sweep-out and --paired-out files."""
    against = args.against or []
    print(f"av reward: {res['av_reward']} av steps: {res['av_steps']}")
    if "latency" in res:
        print(latency_line(res["latency"]))
    if "sensor" in res:
        print(sensor_line(res["sensor"]))
    for k, rec in enumerate(res.get("history", ())):                          # the checkpoints decide: one line per distinct policy
        print(f"history: checkpoint {k}: " + ("none" if rec is None else f"{rec['obs']} observations + {rec['actions']} actions back, {rec['num_obs']} -> {rec['width']} columns"))
    if args.outcomes:
        print("\n".join(outcome_lines(res["outcomes"])) if res["outcomes"]["windows"] > 0 else "no env has reset: no outcome window yet")
    for a, p in enumerate(res["per_agent"]):
        print(f"agent {a}: games {res['games']} reward std {p['reward_std']:.6g} min {p['reward_min']:.6g} max {p['reward_max']:.6g} (av {p['av_reward']:.6g})")
    per_ckpt = len(res.get("groups", ())) // (1 + len(against))               # with --against: cell index -> checkpoint index
    for i, g in enumerate(res.get("groups", ())):
        print((f"checkpoint {i // per_ckpt} " if against else "") + group_line(g))
    if "paired_diff" in res:
        for p in res["paired_diff"]["cells"]:
            print(pair_line(p, res["groups"], res["paired_diff"]["episodes"] * (task.num_envs // len(res["groups"]))))
    if "actuators" in res:
        for g in res["actuators"]["groups"]:
            print(actuator_table(g, "cell " + cell_text(g["cell"])))
        if args.actuators_out:
            with open(args.actuators_out, "w") as fh:
                json.dump(res["actuators"], fh, indent=1)
            print(f"wrote {args.actuators_out}")
    if args.sweep_out:
        with open(args.sweep_out, "w") as fh:                                  # (a cell's latency axes are in its `cell`, as ints)
            json.dump(res["groups"], fh, indent=1)
        print(f"wrote {args.sweep_out}")
    if args.paired_out:
        with open(args.paired_out, "w") as fh:
            json.dump(dict(res["paired_diff"], **{k: res[k] for k in ("latency", "sensor") if k in res}), fh, indent=1)
        print(f"wrote {args.paired_out}")
    print(f"{res['steps_played']} control steps x {task.num_envs} envs in {res['seconds']:.3f} s", flush=True)
    if recorder is not None and args.capture_trajectory:
        print(f"saved {recorder.trajectory.save(args.capture_trajectory, fps=args.capture_fps)} (trajectory)", flush=True)
    if recorder is not None and args.capture:
        files = recorder.save(args.capture, fps=args.capture_fps)
        print(f"captured {res['captured_frames']} frames, kept the last {min(res['captured_frames'], recorder.length)}: {files[0]}" +
              (f" .. {files[-1]}" if len(files) > 1 else ""), flush=True)


def main(argv=None):
    args = parse_args(argv)
    import isaacgym_amd
    from ..policy import RLGamesPolicy
    task_cfg = None
    if args.cfg_dir:
        from .. import cfgyaml
        task_cfg = cfgyaml.compose(args.task, args.cfg_dir, overrides={"num_envs": args.num_envs})["task"]
    task = isaacgym_amd.make(seed=args.seed, task=args.task, num_envs=args.num_envs, cfg=task_cfg)
    policy = RLGamesPolicy.load(args.checkpoint, task.device)
    recorder = make_recorder(task, args) if args.capture or args.capture_trajectory else None
    sweep = Sweep.parse(args.sweep, paired=args.paired) if args.sweep else None
    paired_diff, baseline = args.paired_diff, args.baseline or 0
    if args.against:
        (policy, sweep, baseline), paired_diff = against_cells(args, task, policy, sweep), True
    pl = Player(task, policy, games_num=args.games, deterministic=not args.stochastic, seed=args.seed, poll_every=args.poll_every,
                max_steps=args.max_steps, sigma=args.sigma, recorder=recorder, outcomes=args.outcomes, sweep=sweep, paired_diff=paired_diff,
                baseline=baseline, actuators=actuator_option(args), action_delay=args.action_delay, obs_delay=args.obs_delay,
                **{k: getattr(args, k) for k in SENSOR_AXES + tuple(f"{a}_columns" for a in SENSOR_AXES)})
    last = dict(games=0, steps=0, reward=[0.0])

    def on_poll(tot):                     # rl_games prints `reward: ... steps: ...` per finished batch: here, the games since the last poll
        n = tot["games"] - last["games"]
        if n > 0:
            print(f"reward: {(tot['reward'][0] - last['reward'][0]) / n} steps: {(tot['steps'] - last['steps']) / n}", flush=True)
        last.update(games=tot["games"], steps=tot["steps"], reward=list(tot["reward"]))
        if args.outcomes:
            o = pl.read_outcomes()
            if o["windows"] > 0:
                print("\n".join(outcome_lines(o)), flush=True)

    res = pl.run(on_poll=on_poll)
    print_report(args, task, res, recorder)
    return res
