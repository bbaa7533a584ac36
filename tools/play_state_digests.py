"""Record the bits of the play accounting (isaacgym_amd.play.EpisodeStats) on float rewards: sha256 of each part of state_bytes() after
STEPS accumulates of the tests' recorded sequences, per case, into tests/golden/play_state_digests.json.  The fp64 sum order of the kernels
is a contract (include/ppenv_play.h) that a tolerance cannot hold; tests/test_play_gpu.py::test_state_digests_are_the_recorded_ones compares
against this file.  It was recorded on one MI355X from the commit BEFORE the single and the grouped kernels were folded into one family, and
is recorded again only when the sum order is changed on purpose.  Needs a GPU.

    python tools/play_state_digests.py [--out tests/golden/play_state_digests.json]

Cases: every (num_agents, num_envs) of test_play_host.SHAPES + [(1, 1000), (2, 1000)], once never frozen and once with the games_num of
test_kernel_freeze (half the games the sequence holds), all STEPS steps, so the freeze falls inside the run.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARTS = ("cur_reward", "cur_steps", "totals")


def cases():
    """-> [(key, num_agents, num_envs, games_num, rews, dones)], the sequences as test_kernel_matches_shim_and_loop builds them."""
    import play_shim_binding as ps
    from test_play_host import NEVER, SHAPES, STEPS, rlgames_loop
    out = []
    for num_agents, num_envs in SHAPES + [(1, 1000), (2, 1000)]:
        dones = ps.scripted_dones(STEPS, num_envs, num_agents, words=(1, 2, 1 << 32))
        rews = ps.rewards(STEPS, num_agents * num_envs, seed=6 + num_envs)
        half = max(rlgames_loop(rews, dones, num_agents, NEVER)["games"] // 2, 1)
        for name, games_num in (("never", NEVER), ("freeze", half)):
            out.append((f"{num_agents}x{num_envs}_{name}", num_agents, num_envs, games_num, rews, dones))
    return out


def play(torch, stats, rews, dones):
    """Every step of the sequences into `stats` (accumulate(rew, done), state_bytes()) -> {part: sha256 hex}."""
    from test_play_gpu import device_sequence, run_device
    r, d = device_sequence(torch, rews, dones)
    run_device(torch, stats, r, d)
    return {part: hashlib.sha256(b).hexdigest() for part, b in zip(PARTS, stats.state_bytes())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "play_state_digests.json"))
    args = ap.parse_args()
    import numpy
    import torch
    from isaacgym_amd.play import EpisodeStats
    from test_play_gpu import DEV
    from test_play_host import STEPS
    recorded = {}
    for key, num_agents, num_envs, games_num, rews, dones in cases():
        recorded[key] = dict(games_num=games_num, **play(torch, EpisodeStats(num_envs, num_agents, games_num, DEV), rews, dones))
    with open(args.out, "w") as fh:
        json.dump(dict(made_with=dict(numpy=numpy.__version__, torch=torch.__version__), steps=STEPS, cases=recorded), fh, indent=1)
        fh.write("\n")
    print(f"wrote {len(recorded)} cases to {args.out}")


if __name__ == "__main__":
    main()
