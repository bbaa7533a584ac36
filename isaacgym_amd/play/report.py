"""The player's host arithmetic and text: ctypes structs -> dicts, dicts -> the result's figures, figures -> the CLI's lines.  Nothing
here touches the device."""
import math

from .._lib import MAX_AGENTS, TA_OUTCOME_NAMES

# the reference's five prints (TA:1164-1168), in its order and wording
OUTCOME_PRINTS = (("fall_down", "the sum of the huamnoid which fall down:"), ("closer", "the sum of the envs which are closer to the paddle:"),
                  ("hit_paddle", "the sum of the envs which hit the paddle:"), ("cross_net", "the sum of the envs which cross the net:"),
                  ("hit_table", "the sum of the envs which hit the table:"))
ACT_INT_FIELDS, ACT_SUM_FIELDS, ACT_MAX_FIELDS = ("c_effort", "c_vel", "c_limit", "c_clip"), ("abs_tau", "tau_sq", "power"), ("max_abs_tau", "max_abs_vel", "max_exc")


def _stderr_of_mean(s, sq, n):
    """The standard error of the mean of n values from their sum and their sum of squares: sqrt((sq - s^2 / n) / (n - 1) / n), a negative
    variance estimate (rounding) taken as 0; nan for n < 2."""
    return math.sqrt(max(sq - s * s / n, 0.0) / (n - 1) / n) if n >= 2 else float("nan")


def outcomes_dict(t):
    """A host copy of pp_ta_outcome (TAOutcome) -> dict(windows, envs, the five counts by name, <name>_rate = count / envs — None while
    no window was counted — and last_envs, last_<name>: the most recent window alone)."""
    envs = int(t.envs)
    out = dict(windows=int(t.windows), envs=envs, last_envs=int(t.last_envs))
    for k, name in enumerate(TA_OUTCOME_NAMES):
        out[name] = int(t.count[k])
        out[f"{name}_rate"] = int(t.count[k]) / envs if envs > 0 else None
        out[f"last_{name}"] = int(t.last[k])
    return out


def outcome_lines(o):
    """The reference's five lines for an outcomes dict, as rates of the envs over all windows."""
    return [f"{text} {o[name + '_rate']} of the envs ({o[name]} / {o['envs']} in {o['windows']} windows)" for name, text in OUTCOME_PRINTS]


def totals_dict(t, num_agents=MAX_AGENTS):
    """PlayTotals -> a Python dict (the per-agent fields as lists of num_agents)."""
    return dict(games=int(t.games), steps=int(t.steps), launches=int(t.launches), reward=list(t.reward)[:num_agents],
                reward_sq=list(t.reward_sq)[:num_agents], reward_min=list(t.reward_min)[:num_agents], reward_max=list(t.reward_max)[:num_agents])


def summarize(totals, num_agents=1):
    """The result-dict arithmetic from a totals dict (EpisodeStats.read()): rl_games' av reward = sum_rewards / games_played (agent 0's)
    and av steps = sum_steps / games_played, plus the population standard deviation sqrt(max(E[x^2] - E[x]^2, 0)), minimum and maximum of
    the games' returns; `per_agent`: the four reward figures for each agent.  With no game counted the averages are nan."""
    g = int(totals["games"])
    per_agent = []
    for a in range(num_agents):
        if g > 0:
            mean = totals["reward"][a] / g
            std = math.sqrt(max(totals["reward_sq"][a] / g - mean * mean, 0.0))
        else:
            mean = std = float("nan")
        per_agent.append(dict(av_reward=mean, reward_std=std, reward_min=float(totals["reward_min"][a]), reward_max=float(totals["reward_max"][a])))
    out = dict(games=g, av_steps=totals["steps"] / g if g > 0 else float("nan"))
    out.update(per_agent[0])
    out["per_agent"] = per_agent
    return out


def sum_totals(per_group):
    """A list of totals dicts (GroupStats.read()) -> one totals dict over all groups: counts and sums added in group order (`launches` too:
    group-steps), the extrema merged."""
    A = len(per_group[0]["reward"])
    out = dict(games=0, steps=0, launches=0, reward=[0.0] * A, reward_sq=[0.0] * A, reward_min=[math.inf] * A, reward_max=[-math.inf] * A)
    for t in per_group:
        for k in ("games", "steps", "launches"):
            out[k] += t[k]
        for a in range(A):
            out["reward"][a] += t["reward"][a]
            out["reward_sq"][a] += t["reward_sq"][a]
            out["reward_min"][a] = min(out["reward_min"][a], t["reward_min"][a])
            out["reward_max"][a] = max(out["reward_max"][a], t["reward_max"][a])
    return out


def group_summary(cell, totals, num_agents, games_num, paired=False):
    """One entry of run()'s `groups`: the cell, summarize() of the group's totals, reward_stderr = reward_std / sqrt(games) (nan with no
    game; the UNPAIRED standard error, conservative for a difference of paired cells), complete = games >= games_num and `paired`."""
    out = dict(cell=dict(cell), paired=bool(paired))
    out.update(summarize(totals, num_agents))
    g = out["games"]
    out["reward_stderr"] = out["reward_std"] / math.sqrt(g) if g > 0 else float("nan")
    out["complete"] = g >= int(games_num)
    return out


def pair_totals_dict(t, num_agents=MAX_AGENTS):
    """PlayPairTotals -> a Python dict (the per-agent sums as lists of num_agents; the struct's `cell` and `base` are cell_sum and base_sum)."""
    return dict(pairs=int(t.pairs), steps_diff=int(t.steps_diff), diff=list(t.diff)[:num_agents], diff_sq=list(t.diff_sq)[:num_agents],
                cell_sum=list(t.cell)[:num_agents], base_sum=list(t.base)[:num_agents])


def pair_summary(cell, baseline, totals, num_agents=1):
    """One entry of run()'s paired_diff["cells"] from a pair_totals_dict: over the n = pairs pairs (env i, episode m) both cells played,
    diff = sum(d) / n with d = return(cell) - return(baseline), diff_stderr = sqrt((sum(d^2) - sum(d)^2 / n) / (n - 1) / n) — the standard
    error of the mean of the paired differences, nan for n < 2 — cell_mean and base_mean the two means over the SAME pairs (not the
    av_reward of `groups`, which is over the first games to finish), steps_diff the mean difference of the episode lengths; agent 0's
    figures at the top, all agents' under per_agent.  With no pair the means are nan."""
    n = int(totals["pairs"])
    per_agent = []
    for a in range(num_agents):
        sd, sq = totals["diff"][a], totals["diff_sq"][a]
        per_agent.append(dict(diff=sd / n if n > 0 else float("nan"), diff_stderr=_stderr_of_mean(sd, sq, n),
                              cell_mean=totals["cell_sum"][a] / n if n > 0 else float("nan"), base_mean=totals["base_sum"][a] / n if n > 0 else float("nan")))
    out = dict(cell=int(cell), baseline=int(baseline), pairs=n)
    out.update(per_agent[0])
    out["steps_diff"] = totals["steps_diff"] / n if n > 0 else float("nan")
    out["per_agent"] = per_agent
    return out


def act_totals_dict(group, joints):
    """A PlayActGroup and its D PlayActJoint -> a Python dict: games, samples, launches, energy, energy_sq and, per joint field, a list of D."""
    out = dict(games=int(group.games), samples=int(group.samples), launches=int(group.launches), energy=float(group.energy), energy_sq=float(group.energy_sq))
    for k in ACT_INT_FIELDS:
        out[k] = [int(getattr(j, k)) for j in joints]
    for k in ACT_SUM_FIELDS + ACT_MAX_FIELDS:
        out[k] = [float(getattr(j, k)) for j in joints]
    return out


def sum_act_totals(per_group):
    """A list of act_totals_dict -> one over all groups: counts and sums added in group order, the maxima merged."""
    D = len(per_group[0]["abs_tau"])
    out = dict(games=0, samples=0, launches=0, energy=0.0, energy_sq=0.0, **{k: [0] * D for k in ACT_INT_FIELDS}, **{k: [0.0] * D for k in ACT_SUM_FIELDS},
               max_abs_tau=[0.0] * D, max_abs_vel=[0.0] * D, max_exc=[-math.inf] * D)
    for t in per_group:
        for k in ("games", "samples", "launches", "energy", "energy_sq"):
            out[k] += t[k]
        for d in range(D):
            for k in ACT_INT_FIELDS + ACT_SUM_FIELDS:
                out[k][d] += t[k][d]
            for k in ACT_MAX_FIELDS:
                out[k][d] = max(out[k][d], t[k][d])
    return out


def actuator_summary(totals, limits, names, control_dt):
    """One entry of run()'s actuators["total"] / ["groups"] from an act_totals_dict.  With n = games and s = samples (a game of L control
    steps gives L - 1): energy_per_game [J] = control_dt * energy / n, energy_stderr = control_dt * sqrt((energy_sq - energy^2 / n) / (n - 1) / n)
    (nan for n < 2), mean_power [W] = energy / s — the power term sum_d |tau * qd| averaged over the samples — and `per_joint`, one dict per
    joint: tau_mean_abs, tau_rms, tau_peak [N m], tau_peak_frac = tau_peak / effort, vel_peak [rad / s], vel_peak_frac = vel_peak / vel_limit,
    excursion_max [rad] = the largest of max(lower - q, q - upper) (positive: beyond the limit; -inf with no sample), power_mean [W], and the
    rates over the samples at_effort, at_vel_limit, at_pos_limit, action_clip.  The per-sample figures are nan with no sample."""
    n, s, nan = int(totals["games"]), int(totals["samples"]), float("nan")
    e, dt = totals["energy"], float(control_dt)
    out = dict(games=n, samples=s, energy_per_game=dt * e / n if n > 0 else nan, energy_stderr=dt * _stderr_of_mean(e, totals["energy_sq"], n),
               mean_power=e / s if s > 0 else nan)
    rate = (lambda v: v / s) if s > 0 else (lambda v: nan)
    out["per_joint"] = [dict(joint=names[d], tau_mean_abs=rate(totals["abs_tau"][d]), tau_rms=math.sqrt(rate(totals["tau_sq"][d])) if s > 0 else nan,
                             tau_peak=totals["max_abs_tau"][d], tau_peak_frac=totals["max_abs_tau"][d] / float(limits[d][2]), at_effort=rate(totals["c_effort"][d]),
                             vel_peak=totals["max_abs_vel"][d], vel_peak_frac=totals["max_abs_vel"][d] / float(limits[d][3]), at_vel_limit=rate(totals["c_vel"][d]),
                             at_pos_limit=rate(totals["c_limit"][d]), excursion_max=totals["max_exc"][d], power_mean=rate(totals["power"][d]),
                             action_clip=rate(totals["c_clip"][d])) for d in range(len(names))]
    return out


def cell_text(cell):
    return " ".join(f"{k}={v:g}" if not isinstance(v, (tuple, list)) else f"{k}={v[0]:g}..{v[1]:g}" for k, v in cell.items()) or "(plain)"


def group_line(g):
    """The CLI's line for one entry of `groups`."""
    return (f"cell {cell_text(g['cell'])}: games {g['games']} av reward {g['av_reward']:.6g} +- {g['reward_stderr']:.3g} av steps {g['av_steps']:.6g} "
            f"min {g['reward_min']:.6g} max {g['reward_max']:.6g}" + ("" if g["complete"] else " (incomplete)"))


def pair_line(p, groups, full):
    """The CLI's line for one entry of paired_diff["cells"]; groups: the result's `groups` (the cells' texts), full: the S * M pairs a
    complete cell has."""
    return (f"cell {p['cell']} {cell_text(groups[p['cell']]['cell'])}: vs cell {p['baseline']}: pairs {p['pairs']} diff {p['diff']:.6g} +- {p['diff_stderr']:.3g} "
            f"(cell {p['cell_mean']:.6g}, base {p['base_mean']:.6g}) steps diff {p['steps_diff']:.6g}" + ("" if p["pairs"] == full else " (incomplete)"))


def actuator_table(entry, title=""):
    """The CLI's table for one entry of actuators["groups"] (or its total): a head line, then one row per joint."""
    lines = [f"actuators {title}: games {entry['games']} samples {entry['samples']} energy/game {entry['energy_per_game']:.6g} +- {entry['energy_stderr']:.3g} J "
             f"mean power {entry['mean_power']:.6g} W",
             f"  {'joint':<28}{'|tau| mean':>11}{'rms':>9}{'peak':>9}{'/effort':>8}{'at eff':>8}{'vel peak':>10}{'/limit':>8}{'at vel':>8}{'at pos':>8}"
             f"{'exc max':>9}{'power':>9}{'act clip':>9}"]
    for j in entry["per_joint"]:
        lines.append(f"  {j['joint']:<28}{j['tau_mean_abs']:>11.4g}{j['tau_rms']:>9.4g}{j['tau_peak']:>9.4g}{j['tau_peak_frac']:>8.3f}{j['at_effort']:>8.3f}"
                     f"{j['vel_peak']:>10.4g}{j['vel_peak_frac']:>8.3f}{j['at_vel_limit']:>8.3f}{j['at_pos_limit']:>8.3f}{j['excursion_max']:>9.3g}"
                     f"{j['power_mean']:>9.4g}{j['action_clip']:>9.3f}")
    return "\n".join(lines)


def latency_line(lat):
    """The CLI's head line for run()'s `latency`: per axis the cells' delays in control steps and in milliseconds."""
    from .sweep import DELAY_AXES                                          # (sweep sits above this module: it is read when a line is asked for)
    ms = 1000.0 * lat["control_dt"]
    return f"latency: control dt {ms:.6g} ms; " + "; ".join(
        f"{axis} {','.join(str(k) for k in lat[axis])} steps = {','.join(f'{k * ms:.6g}' for k in lat[axis])} ms" for axis in DELAY_AXES)


def sensor_line(sen):
    """The CLI's head line for run()'s `sensor`: per axis the cells' levels, then the column specs that were given."""
    from .sweep import SENSOR_AXES
    cols = "".join(f"; {k} {v}" for k, v in sen.get("columns", {}).items() if v)
    return "sensor: " + "; ".join(f"{axis} {','.join(f'{v:g}' for v in sen[axis])}" for axis in SENSOR_AXES) + cols
